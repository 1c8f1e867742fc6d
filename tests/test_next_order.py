"""The device successor stage's arithmetic (zeroskip_amd/csrc/zscrc_next_order.h,
the functions the kernels of zscrc_next.hip call) on the CPU: a stand-alone
program (tests/c/next_order.cpp) runs each case of tests/next_cases.py through
them -- the cursors through a table into the level-major matrix, the step, the
stop rule, the filler -- at 1, 2, 64, 1,024 (the default) and 2,048 splitters
and compares rows, seqs, cursors and result words with the Python model's.
The program is built with the address and undefined-behaviour sanitizers and
runs as its own process; nothing is preloaded and nothing of it is loaded into
python.  No GPU."""
import subprocess

import numpy as np
import pytest

from tests import cprog
from tests import next_cases as nc

NO_COMPARE = nc.NO_COMPARE
program = cprog.program_fixture("next_order")


def _run(program, tmp_path, case, setting=(1, False, False, 0), shift=0, qshift=0, want=None):
    path = str(tmp_path / "case.bin")
    with open(path, "wb") as fh:
        fh.write(case.case_file(*setting, shift=shift, qshift=qshift, want=want))
    r = subprocess.run([program[0], path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (case.name, setting, shift, qshift, r.stdout[-500:], r.stderr[-3000:])
    assert r.stdout.startswith("ok %d records %d queries" % (case.n, len(case.queries)))


@pytest.fixture(scope="module")
def cases():
    return nc.small_cases()


def test_sanitizers_are_linked(program):
    """The build with -fsanitize=address,undefined succeeded (without it the
    cases below still compare every word, but see no access outside an array)."""
    assert program[1]


def test_every_small_case(program, cases, tmp_path):
    names = [c.name for c in cases]
    assert len(set(names)) == len(names) >= 40
    for case in cases:
        for setting in nc.settings(case):
            _run(program, tmp_path, case, setting)


@pytest.mark.parametrize("shift", range(1, 8))
def test_source_and_query_address_residues(program, cases, tmp_path, shift):
    """Keys and queries at every offset mod 8 from a source and a query blob at every address mod 8."""
    for case in cases:
        if case.name.startswith("residue") or case.name in ("key_lengths", "shared_prefix"):
            _run(program, tmp_path, case, (3, bool(shift & 1), bool(shift & 2), 0), shift, (shift * 3) % 8)


def test_level_sizes_around_the_table_sizes(program, tmp_path):
    for case in nc.table_cases():
        _run(program, tmp_path, case, (2, False, False, 0))
        _run(program, tmp_path, case, (1, True, True, 0))


def test_a_thousand_deletes(program, tmp_path):
    case = nc.delete_run_case(1000)
    for setting in nc.settings(case):
        _run(program, tmp_path, case, setting)


def test_random_cases(program, tmp_path):
    for seed, case in enumerate(nc.random_cases()):
        _run(program, tmp_path, case, (1 + 3 * seed, bool(seed & 1), bool(seed & 2), seed), seed, 7 - seed)


def test_a_wrong_row_is_seen(program, cases, tmp_path):
    """The comparison has teeth: the older level's record expected instead of
    the newer one's, a row in a filler slot, a wrong seq, a wrong cursor and a
    wrong count each fail the run."""
    case = next(c for c in cases if c.name == "winners")
    setting = (3, False, False, 0)
    rows, seqs, cur, res = case.model(*setting)
    _run(program, tmp_path, case, setting, want=(rows, seqs, cur, res))
    keys = [case.src[int(r[0]):int(r[0]) + int(r[1])] if int(r[0]) != nc.NONE else None for r in rows.reshape(-1, 4)]
    at = keys.index(b"k.value-over-del")
    lv2 = case.levels[2][0]
    older = rows.copy()
    older.reshape(-1, 4)[at] = lv2[[i for i, r in enumerate(lv2) if int(r[2]) == nc.U64_MAX and
                                    int(r[1]) == len(b"k.value-over-del")][0]]
    with pytest.raises(AssertionError):
        _run(program, tmp_path, case, setting, want=(older, seqs, cur, res))
    filled = rows.copy()
    slot = keys.index(None)
    filled.reshape(-1, 4)[slot] = rows.reshape(-1, 4)[at]
    with pytest.raises(AssertionError):
        _run(program, tmp_path, case, setting, want=(filled, seqs, cur, res))
    wrong_seq = seqs.copy()
    wrong_seq.reshape(-1)[at] += np.uint64(1)
    with pytest.raises(AssertionError):
        _run(program, tmp_path, case, setting, want=(rows, wrong_seq, cur, res))
    wrong_cur = cur.copy()
    wrong_cur[0, 3] = nc.END if int(cur[0, 3]) != nc.END else nc.PAGE
    with pytest.raises(AssertionError):
        _run(program, tmp_path, case, setting, want=(rows, seqs, wrong_cur, res))
    for word in (2, 3, 4, 5, 10):
        wrong = list(res)
        wrong[word] += 1
        with pytest.raises(AssertionError):
            _run(program, tmp_path, case, setting, want=(rows, seqs, cur, wrong))


def test_a_record_outside_the_source_is_refused(program, tmp_path):
    case, _ = nc.bad_record_case()
    with pytest.raises(AssertionError):
        _run(program, tmp_path, case, want=NO_COMPARE)


def test_a_level_that_does_not_ascend_stays_inside_its_arrays(program, tmp_path):
    """Without CHECK_ORDER such a level is stepped through all the same: the
    program checks every position against its array and that no query takes
    more steps than there are records, the sanitizers the rest.  With expected
    words the same case is refused as not ascending."""
    case = nc.unordered_case()
    for setting in ((1, False, False, 0), (64, True, True, 0), (3, False, True, 2)):
        for shift in (0, 3):
            _run(program, tmp_path, case, setting, shift, shift, want=NO_COMPARE)
    for seed in range(3):
        _run(program, tmp_path, nc.shuffled_case(seed), (1 + 31 * seed, bool(seed & 1), True, 0), seed, seed + 2,
             want=NO_COMPARE)
    with pytest.raises(AssertionError):
        _run(program, tmp_path, case, want=case.model())
