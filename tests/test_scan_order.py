"""The device prefix scan's arithmetic (zeroskip_amd/csrc/zscrc_scan_order.h,
the functions the kernels of zscrc_scan.hip call) on the CPU: a stand-alone
program (tests/c/scan_order.cpp) scans each case of tests/scan_cases.py through
them -- the bounds through a table, the candidate decomposition, the rank, the
guard and the compaction order -- at 1, 2, 64, 1,024 (the default) and 2,048
splitters and compares
rows, offsets and seqs with the Python model's.  The program is built with the
address and undefined-behaviour sanitizers and runs as its own process;
nothing is preloaded and nothing of it is loaded into python.  No GPU."""
import subprocess

import numpy as np
import pytest

from tests import cprog
from tests import scan_cases as sc

NO_COMPARE = sc.NO_COMPARE
program = cprog.program_fixture("scan_order")


def _run(program, tmp_path, case, keep=False, shift=0, qshift=0, want=None):
    path = str(tmp_path / "case.bin")
    with open(path, "wb") as fh:
        fh.write(case.case_file(keep, shift, qshift, want))
    r = subprocess.run([program[0], path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (case.name, keep, shift, qshift, r.stdout[-500:], r.stderr[-3000:])
    assert r.stdout.startswith("ok %d records %d queries" % (case.n, len(case.queries)))


@pytest.fixture(scope="module")
def cases():
    return sc.small_cases()


def test_sanitizers_are_linked(program):
    """The build with -fsanitize=address,undefined succeeded (without it the
    cases below still compare every row, but see no access outside an array)."""
    assert program[1]


def test_every_small_case(program, cases, tmp_path):
    names = [c.name for c in cases]
    assert len(set(names)) == len(names) >= 40
    for case in cases:
        for keep in (False, True):
            _run(program, tmp_path, case, keep)


@pytest.mark.parametrize("shift", range(1, 8))
def test_source_and_prefix_address_residues(program, cases, tmp_path, shift):
    """Keys and prefixes at every offset mod 8, the long prefixes and the
    zero-padding keys, from a source and a prefix blob at every address mod 8."""
    for case in cases:
        if case.name.startswith("residue") or case.name in ("long_prefixes", "prefixes"):
            _run(program, tmp_path, case, bool(shift & 1), shift, (shift * 3) % 8)


def test_counts_around_the_table_sizes(program, tmp_path):
    for case in sc.table_cases():
        _run(program, tmp_path, case)


def test_candidates_around_the_grid(program, tmp_path):
    """C one below, at and one above the rank's persistent grid."""
    for case in sc.grid_cases():
        _run(program, tmp_path, case, True)


def test_random_cases(program, tmp_path):
    for seed, case in enumerate(sc.random_cases()):
        _run(program, tmp_path, case, bool(seed & 1), seed, 7 - seed)


def test_a_wrong_row_is_seen(program, cases, tmp_path):
    """The comparison has teeth: the older level's value expected instead of
    the newer one's, a row too many in a query, a wrong seq each fail the run."""
    case = next(c for c in cases if c.name == "winners")
    rows, offs, seqs, _ = case.model(False)
    _run(program, tmp_path, case, want=(rows, offs, seqs, None))
    older = rows.copy()
    at = [i for i, r in enumerate(rows) if case.src[int(r[2]):int(r[2]) + int(r[3])] == b"new"][0]
    lv2 = case.levels[2][0]
    older[at] = lv2[[i for i, r in enumerate(lv2) if int(r[2]) == sc.U64_MAX and int(r[1]) == int(rows[at, 1])][0]]
    with pytest.raises(AssertionError):
        _run(program, tmp_path, case, want=(older, offs, seqs, None))
    shifted = offs.copy()
    shifted[1] += np.uint64(1)
    with pytest.raises(AssertionError):
        _run(program, tmp_path, case, want=(rows, shifted, seqs, None))
    wrong_seq = seqs.copy()
    wrong_seq[-1] += np.uint64(1)
    with pytest.raises(AssertionError):
        _run(program, tmp_path, case, want=(rows, offs, wrong_seq, None))


def test_a_record_outside_the_source_is_refused(program, tmp_path):
    case, _ = sc.bad_record_case()
    with pytest.raises(AssertionError):
        _run(program, tmp_path, case, want=NO_COMPARE)


def test_a_level_that_does_not_ascend_stays_inside_its_arrays(program, tmp_path):
    """Without CHECK_ORDER such a level is scanned all the same: the program
    checks every position against its array, the sanitizers the rest.  With
    expected rows the same case is refused as not ascending."""
    case = sc.unordered_case()
    for keep in (False, True):
        for shift in (0, 3):
            _run(program, tmp_path, case, keep, shift, shift, want=NO_COMPARE)
    for seed in range(3):
        _run(program, tmp_path, sc.shuffled_case(seed), bool(seed & 1), seed, seed + 2, want=NO_COMPARE)
    with pytest.raises(AssertionError):
        _run(program, tmp_path, case, want=(sc.recs_of([]), np.zeros(len(case.queries) + 1, np.uint64), [], None))
