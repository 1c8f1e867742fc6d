"""The device packer's layout arithmetic (zeroskip_amd/csrc/zscrc_pack_layout.h,
the functions the kernels of zscrc_devpack.hip call) on the CPU: a stand-alone
program (tests/c/pack_layout.cpp) rebuilds the packed file of each record list
of tests/pack_cases.py through them and the tile sweep of pack_copy_kernel
(zscrc_copy_tiles.h: the run of tiles of a workgroup, the 16-byte word, the
advance, with the lanes played by a loop), at tile sizes 64, 128, 4096 and
65536 and grids of 1, 2, 7 and one more workgroup than tiles, and compares it
with the format oracle's file.  The program is
built with the address and undefined-behaviour sanitizers and runs as its own
process; nothing is preloaded and nothing of it is loaded into python.  No GPU."""
import re
import struct
import subprocess

import pytest

from tests import cprog
from tests import pack_cases as pc

program = cprog.program_fixture("pack_layout")


def _run(program, tmp_path, case, shift):
    path = str(tmp_path / "case.bin")
    want = case.want
    with open(path, "wb") as fh:
        fh.write(struct.pack("<6Q", len(case.src), len(case.recs), len(want), shift, case.startidx, case.endidx))
        fh.write(case.uuid + case.src + case.recs.tobytes() + want)
    r = subprocess.run([program[0], path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (case.name, shift, r.stdout[-500:], r.stderr[-3000:])
    assert r.stdout.startswith("ok %d records %d bytes" % (len(case.recs), len(want)))
    return _stores(r.stdout)


def _stores(line):
    """The stores the ok line counts: (of 16 bytes, of a first half, of a second half)."""
    m = re.search(r"stores: (\d+) of 16 bytes, (\d+) of a first half, (\d+) of a second half", line)
    assert m, line
    return tuple(int(g) for g in m.groups())


@pytest.fixture(scope="module")
def cases():
    return pc.small_cases()


def test_sanitizers_are_linked(program):
    """The build with -fsanitize=address,undefined succeeded (without it the
    cases below still compare every byte, but see no read outside the source)."""
    assert program[1]


def test_every_small_case(program, cases, tmp_path):
    names = [c.name for c in cases]
    assert len(set(names)) == len(names) >= 18
    stores = [_run(program, tmp_path, case, shift=0) for case in cases]
    # the region starts at offset 40, 8 mod 16: its first word is the second
    # half of a 16-byte word in every list that has a record, and where it ends
    # at 8 mod 16 its last word is a first half
    assert all(s[2] > 0 for case, s in zip(cases, stores) if len(case.recs))
    assert sum(s[0] for s in stores) > 0 and sum(s[1] for s in stores) > 0


@pytest.mark.parametrize("shift", range(1, 8))
def test_source_address_residues(program, cases, tmp_path, shift):
    """The alignment grid and the shared-bytes list from a source at every address mod 8."""
    for case in cases:
        if case.name in ("alignment_grid", "shared_bytes", "single_kv", "long_delete"):
            _run(program, tmp_path, case, shift)


def test_a_wrong_byte_is_seen(program, cases, tmp_path):
    """The comparison has teeth: one byte of the expected file changed fails the run."""
    case = next(c for c in cases if c.name == "single_kv")
    bad = pc.Case("single_kv_wrong", case.src, case.recs, want=case.want[:64] + bytes([case.want[64] ^ 1]) + case.want[65:])
    with pytest.raises(AssertionError):
        _run(program, tmp_path, bad, 0)
