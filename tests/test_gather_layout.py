"""The value gather's shared arithmetic (zeroskip_amd/csrc/zscrc_gather_layout.h,
the functions the kernels of zscrc_gather.hip and zscrc_zs_gather call) on the
CPU: a stand-alone program (tests/c/gather_layout.cpp) gathers each case of
tests/gather_cases.py through them -- the kinds, the bounds check, the
saturating prefix, the word builder both carried along and searched for --
and compares the bytes with the Python model's.  The program is built with the
address and undefined-behaviour sanitizers and runs as its own process;
nothing is preloaded and nothing of it is loaded into python.  No GPU."""
import subprocess

import pytest

from tests import cprog
from tests import gather_cases as gc

program = cprog.program_fixture("gather_layout")


def _run(program, tmp_path, case, shift=0, want=None):
    path = str(tmp_path / "case.bin")
    with open(path, "wb") as fh:
        fh.write(case.case_file(shift, want))
    r = subprocess.run([program[0], path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (case.name, shift, r.stdout[-500:], r.stderr[-3000:])
    assert r.stdout.startswith("ok %d items" % case.nq)


@pytest.fixture(scope="module")
def cases():
    return gc.small_cases()


def test_sanitizers_are_linked(program):
    """The build with -fsanitize=address,undefined succeeded (without it the
    cases below still compare every byte, but see no read outside the source)."""
    assert program[1]


def test_every_small_case(program, cases, tmp_path):
    names = [c.name for c in cases]
    assert len(set(names)) == len(names) >= 35
    for case in cases:
        _run(program, tmp_path, case)


@pytest.mark.parametrize("shift", range(8))
def test_source_address_residues(program, cases, tmp_path, shift):
    """Sources at every address mod 8: values from every offset, values that
    end with the source's last byte, empty items at both ends of the list."""
    for case in cases:
        if case.name in ("ends", "front", "lengths64", "n257") or case.name.startswith("tile64_r"):
            _run(program, tmp_path, case, shift)


def test_random_cases(program, tmp_path):
    for seed in range(3):
        _run(program, tmp_path, gc.random_case(seed, 500), seed + 1)


def test_a_wrong_byte_is_seen(program, cases, tmp_path):
    """The comparison has teeth: one expected byte changed fails the run, the first and the last one too."""
    case = next(c for c in cases if c.name == "ends")
    want = case.model(crcs=False)[0].tobytes()
    _run(program, tmp_path, case, want=want)
    for at in (0, len(want) // 2, len(want) - 1):
        bad = bytearray(want)
        bad[at] ^= 0x40
        with pytest.raises(AssertionError):
            _run(program, tmp_path, case, want=bytes(bad))
    with pytest.raises(AssertionError):
        _run(program, tmp_path, case, want=want + b"\0")       # a wrong total


def test_a_value_one_byte_past_the_source_is_refused(program, cases, tmp_path):
    case = next(c for c in cases if c.name == "ends")
    size = len(case.src)
    for off, ln in ((size - 29, 30), (size, 1), (size + 1, 0), (1, size), (5, 1 << 63), (gc.U64_MAX - 1, 2)):
        items = case.items.copy()
        items[2, 2:] = (off, ln)
        with pytest.raises(AssertionError):
            _run(program, tmp_path, gc.GatherCase("outside", case.src, items), want=b"")
    # the same words under a miss or a bad query are never looked at
    items = case.items.copy()
    items[2] = gc.WILD_MISS
    items[3] = gc.WILD_BADQ
    _run(program, tmp_path, gc.GatherCase("wild", case.src, items))
