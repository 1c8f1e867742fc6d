"""The device merge's order arithmetic (zeroskip_amd/csrc/zscrc_merge_order.h,
the functions the kernels of zscrc_merge.hip call) on the CPU: a stand-alone
program (tests/c/merge_order.cpp) merges each case of tests/merge_cases.py
through them -- rebase, sort entries, the tile sort's network, the passes cut
by diagonal searches, the winner rule -- at tiles of 64 and 256 entries and
compares the winners with the list the Python model gives.  The program is
built with the address and undefined-behaviour sanitizers and runs as its own
process; nothing is preloaded and nothing of it is loaded into python.  No GPU."""
import subprocess

import numpy as np
import pytest

from tests import cprog
from tests import merge_cases as mc

program = cprog.program_fixture("merge_order")


def _run(program, tmp_path, case, shift, drop, want=None):
    path = str(tmp_path / "case.bin")
    with open(path, "wb") as fh:
        fh.write(case.case_file(shift, drop, want))
    n_want = len(case.model(drop)[0] if want is None else want)
    r = subprocess.run([program[0], path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (case.name, shift, drop, r.stdout[-500:], r.stderr[-3000:])
    assert r.stdout.startswith("ok %d records %d winners" % (case.n, n_want))


@pytest.fixture(scope="module")
def cases():
    return mc.small_cases()


def test_sanitizers_are_linked(program):
    """The build with -fsanitize=address,undefined succeeded (without it the
    cases below still compare every winner, but see no read outside the source)."""
    assert program[1]


def test_every_small_case(program, cases, tmp_path):
    names = [c.name for c in cases]
    assert len(set(names)) == len(names) >= 30
    for case in cases:
        for drop in (False, True):
            _run(program, tmp_path, case, 0, drop)


@pytest.mark.parametrize("shift", range(1, 8))
def test_source_address_residues(program, cases, tmp_path, shift):
    """Keys at every offset mod 8, the key that ends with the source and the
    long keys from a source at every address mod 8."""
    for case in cases:
        if case.name.startswith("residue") or case.name in ("ends_at_last_byte", "long_keys", "key_lengths",
                                                            "shared_prefix"):
            _run(program, tmp_path, case, shift, False)


def test_random_cases(program, tmp_path):
    for seed in range(4):
        case = mc.random_case(seed)
        _run(program, tmp_path, case, seed, bool(seed & 1))


def test_a_wrong_winner_is_seen(program, cases, tmp_path):
    """The comparison has teeth: the earlier record of a key expected instead of the later fails the run."""
    case = next(c for c in cases if c.name == "deletes")
    want, _ = case.model(False)
    recs = case.rebased()
    assert want[0].tolist() == recs[4].tolist()         # key a: the delete of list 1 wins over list 0's value
    bad = want.copy()
    bad[0] = recs[0]
    _run(program, tmp_path, case, 0, False, want=want)
    with pytest.raises(AssertionError):
        _run(program, tmp_path, case, 0, False, want=bad)


def test_a_record_outside_the_source_is_refused(program, cases, tmp_path):
    case = next(c for c in cases if c.name == "one_record")
    recs = case.lists[0][0].copy()
    recs[0, 1] = len(case.src) - int(recs[0, 0]) + 1    # the key ends one byte past the source
    bad = mc.Case("outside", case.src, [(recs, 0)])
    with pytest.raises(AssertionError):
        _run(program, tmp_path, bad, 0, False, want=np.zeros((0, 4), np.uint64))
