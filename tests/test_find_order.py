"""The device lookup's search arithmetic (zeroskip_amd/csrc/zscrc_find_order.h,
the functions the kernels of zscrc_find.hip call) on the CPU: a stand-alone
program (tests/c/find_order.cpp) searches each case of tests/find_cases.py
through them -- rebase, the order check, splitter positions, the tables, the
bucket and the bisection inside it -- at 1, 2, 64 and 2,048 splitters and
compares the hits with the Python model's.  The program is built with the
address and undefined-behaviour sanitizers and runs as its own process;
nothing is preloaded and nothing of it is loaded into python.  No GPU."""
import subprocess

import numpy as np
import pytest

from tests import cprog
from tests import find_cases as fc

program = cprog.program_fixture("find_order")


def _run(program, tmp_path, case, shift=0, qshift=0, want=None):
    path = str(tmp_path / "case.bin")
    with open(path, "wb") as fh:
        fh.write(case.case_file(shift, qshift, want))
    r = subprocess.run([program[0], path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (case.name, shift, qshift, r.stdout[-500:], r.stderr[-3000:])
    assert r.stdout.startswith("ok %d records %d queries" % (case.n, len(case.queries)))


@pytest.fixture(scope="module")
def cases():
    return fc.small_cases()


def test_sanitizers_are_linked(program):
    """The build with -fsanitize=address,undefined succeeded (without it the
    cases below still compare every hit, but see no read outside the source)."""
    assert program[1]


def test_every_small_case(program, cases, tmp_path):
    names = [c.name for c in cases]
    assert len(set(names)) == len(names) >= 25
    for case in cases:
        _run(program, tmp_path, case)


@pytest.mark.parametrize("shift", range(1, 8))
def test_source_and_query_address_residues(program, cases, tmp_path, shift):
    """Keys at every offset mod 8, the key that ends with the source and the
    long keys, from a source and a query blob at every address mod 8."""
    for case in cases:
        if case.name.startswith("residue") or case.name in ("ends_at_last_byte", "long_keys", "key_lengths",
                                                            "shared_prefix"):
            _run(program, tmp_path, case, shift, (shift * 3) % 8)


def test_counts_around_the_table_sizes(program, tmp_path):
    """S - 1, S, S + 1, 2 S + 1 and 3 (S + 1) - 1 records for S = 2, 64 and 2,048 (fewer records than splitters too)."""
    for n in (6, 7, 127, 128, 2047, 2049, 4097):
        _run(program, tmp_path, fc.counted_case(n))


def test_random_cases(program, tmp_path):
    for seed in range(4):
        _run(program, tmp_path, fc.random_find_case(seed), seed, 7 - seed)


def test_a_wrong_hit_is_seen(program, cases, tmp_path):
    """The comparison has teeth: the older level's value expected instead of the newer level's delete fails the run."""
    case = next(c for c in cases if c.name == "deletes")
    want, _ = case.model()
    assert int(want[0, 0]) == 0 and int(want[0, 2]) == fc.U64_MAX      # key a: level 0's delete
    bad = want.copy()
    older = case.levels[2][0][0]                                        # key a in level 2
    bad[0] = (2, 0, int(older[2]), int(older[3]))
    _run(program, tmp_path, case, want=want)
    with pytest.raises(AssertionError):
        _run(program, tmp_path, case, want=bad)
    off_by_one = want.copy()
    off_by_one[3, 1] += np.uint64(1)                                    # key d: the lower bound in the last level
    with pytest.raises(AssertionError):
        _run(program, tmp_path, case, want=off_by_one)


def test_a_record_outside_the_source_is_refused(program, cases, tmp_path):
    case = next(c for c in cases if c.name == "n1")
    recs = case.levels[0][0].copy()
    recs[0, 1] = len(case.src) - int(recs[0, 0]) + 1    # the key ends one byte past the source
    bad = fc.FindCase("outside", case.src, [(recs, 0)], case.qsrc, case.queries)
    with pytest.raises(AssertionError):
        _run(program, tmp_path, bad, want=np.zeros((len(case.queries), 4), np.uint64))
