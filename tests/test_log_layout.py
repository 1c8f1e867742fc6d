"""The device log writer's layout arithmetic (zeroskip_amd/csrc/
zscrc_log_layout.h and zscrc_pack_layout.h, the functions the kernels of
zscrc_devlog.hip call) on the CPU: a stand-alone program (tests/c/
log_layout.cpp) rebuilds the image of each small case of tests/log_cases.py
through them and the tile sweep of log_copy_kernel (zscrc_copy_tiles.h: the run
of tiles of a workgroup, the 16-byte word, the advance, with the lanes played
by a loop), at tile sizes 64, 128, 4096 and 65536 and grids of 1, 2, 7 and one
more workgroup than tiles, and compares it with the format oracle's image.  The program is built with the address and
undefined-behaviour sanitizers and runs as its own process; nothing is
preloaded and nothing of it is loaded into python.  No GPU."""
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import cprog
from tests import log_cases as lc

NO_TABLE = (1 << 64) - 1
program = cprog.program_fixture("log_layout")


def _run(program, tmp_path, case, shift, want=None):
    path = str(tmp_path / "case.bin")
    want = case.want if want is None else want
    te = [] if case.tx_end is None else case.tx_end
    with open(path, "wb") as fh:
        fh.write(struct.pack("<10Q", len(case.src), case.n, NO_TABLE if case.tx_end is None else len(te), case.at,
                             int(case.finalise), case.prev_crc, len(want), shift, case.startidx, case.endidx))
        fh.write(case.uuid + case.src + case.recs.tobytes() + np.asarray(te, np.uint64).tobytes() + want)
    r = subprocess.run([program[0], path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (case.name, shift, r.stdout[-500:], r.stderr[-3000:])
    assert r.stdout.startswith("ok %d records %d commits %d bytes" % (case.n, case.n_commits, len(want)))
    m = re.search(r"stores: (\d+) of 16 bytes, (\d+) of a first half, (\d+) of a second half", r.stdout)
    assert m, r.stdout
    return tuple(int(g) for g in m.groups())


def test_sanitizers_are_linked(program):
    """The build with -fsanitize=address,undefined succeeded (without it the
    cases below still compare every byte, but see no read outside the source)."""
    assert program[1]


def test_every_small_case(program, tmp_path):
    cases = lc.small_cases()
    assert len(cases) >= 160
    for case in cases:
        stores = _run(program, tmp_path, case, shift=0)
        if case.name == "append_at_8_mod_16":
            # records from 8 mod 16 on: the first one begins with a second half
            assert stores[0] > 0 and stores[2] > 0, stores


def test_every_kind_of_store(program, tmp_path):
    """An append at 8 mod 16 whose third transaction is a delete of 40 bytes
    from 0 mod 16 on (a record of 56 bytes and two commits of 8 before it): the word that holds the delete's last 8 bytes and
    its commit is a store of the first half alone (append_at_8_mod_16 itself
    has no record that ends at 8 mod 16 in front of a commit); the first
    record's first word is a second half."""
    pre = lc.earlier_image(False)
    case = lc.from_lengths("append_first_half", [(4, 4), (9, None)], seed=27, tx_end=[1, 1, 2], prefix=pre)
    assert len(pre) % 16 == 8 and len(case.want) == len(pre) + 56 + 8 + 8 + 40 + 8
    assert min(_run(program, tmp_path, case, shift=0)) > 0


@pytest.mark.parametrize("shift", range(1, 8))
def test_source_address_residues(program, tmp_path, shift):
    """The alignment grid, the shared bytes and the re-logged image from a source at every address mod 8."""
    for case in lc.small_cases():
        if case.name in ("alignment_grid", "shared_bytes", "single_kv", "src_inside_out", "tx_two_deletes",
                         "count_130", "append_at_8_mod_16"):
            _run(program, tmp_path, case, shift)


def test_long_span_of_small_records(program, tmp_path):
    """The 24-byte commit of a span above 16,777,215 bytes, across a 64 KiB tile edge."""
    case = next(c for c in lc.big_cases() if c.name == "long_span_small_records")
    _run(program, tmp_path, case, 5)


def test_a_wrong_byte_is_seen(program, tmp_path):
    """The comparison has teeth: one byte of the expected image changed fails the run."""
    case = next(c for c in lc.small_cases() if c.name == "single_kv")
    w = case.want
    with pytest.raises(AssertionError):
        _run(program, tmp_path, case, 0, want=w[:70] + bytes([w[70] ^ 1]) + w[71:])
