"""zscrc_device_gather's argument checks and its scratch size (no GPU: all of
them return before any device call), and the same checks of zscrc_zs_gather."""
import ctypes

from zeroskip_amd import zsfile
from zeroskip_amd._lib import lib

EINVAL = -1
SRC = 0x10000  # never dereferenced: the calls below fail their argument checks
ITEMS = 0x20000
OUT = 0x80000
OFFS = 0x40000
RES = 0x50000
N_MAX = (1 << 31) - 1


def _gather(src=SRC, src_size=4096, items=ITEMS, nq=2, out=OUT, cap=256, offs=OFFS, crcs=None, res=RES, scratch=None,
            tile=None, flags=0):
    return lib().zscrc_device_gather(src, src_size, items, nq, out, cap, offs, crcs, res, scratch,
                                     None if tile is None else ctypes.byref(zsfile.GatherOpts(tile)), flags, None)


def test_bad_arguments_are_einval():
    assert _gather(res=None) == EINVAL
    assert _gather(items=None) == EINVAL                  # nq > 0 needs the items
    assert _gather(offs=None) == EINVAL                   # and the offsets
    assert _gather(offs=None, nq=0, items=None) == EINVAL  # nq = 0 too: offs receives the one word
    assert _gather(src=None) == EINVAL                    # src_size > 0 needs the source
    assert _gather(out=None) == EINVAL                    # out_cap > 0 needs the output
    for off in (1, 4, 8):
        assert _gather(out=OUT + off) == EINVAL, off      # d_out not 16-byte aligned
        assert _gather(out=OUT + off, cap=0) == EINVAL, off
        assert _gather(scratch=OUT + off) == EINVAL, off  # nor the scratch
    for flags in (1, 2, 4, 1 << 31):
        assert _gather(flags=flags) == EINVAL, flags      # no flag is defined
    for t in (1, 32, 48, 96, 3000, 65537, 1 << 17, 1 << 40):
        assert _gather(tile=t) == EINVAL, t               # not a power of two, or outside 64 .. 65536
    assert _gather(nq=N_MAX + 1) == EINVAL                # the stated limits
    assert _gather(nq=(1 << 64) - 1) == EINVAL
    assert _gather(src_size=(1 << 62) + 1) == EINVAL


def test_an_output_that_overlaps_the_source_is_einval():
    assert _gather(src=SRC, src_size=4096, out=SRC, cap=16) == EINVAL
    assert _gather(src=SRC, src_size=4096, out=SRC + 4080, cap=256) == EINVAL      # the source's last 16 bytes
    assert _gather(src=SRC + 16, src_size=4096, out=SRC - 240, cap=272) == EINVAL  # the output's last 16 bytes
    assert _gather(src=SRC, src_size=1 << 40, out=SRC + (1 << 30), cap=16) == EINVAL
    assert _gather(out=16, cap=(1 << 64) - 16) == EINVAL                            # an output that would wrap


def test_the_host_gather_checks_the_same_arguments():
    def host(src=SRC, src_size=4096, items=ITEMS, nq=2, out=OUT, cap=256, offs=OFFS, crcs=None, res=RES):
        return lib().zscrc_zs_gather(src, src_size, items, nq, out, cap, offs, crcs, res)

    for bad in (dict(res=None), dict(items=None), dict(offs=None), dict(offs=None, nq=0, items=None), dict(src=None),
                dict(out=None), dict(nq=N_MAX + 1), dict(src_size=(1 << 62) + 1), dict(out=SRC, cap=16),
                dict(out=SRC + 4080)):
        assert host(**bad) == EINVAL, bad


def test_scratch_bytes():
    for t in (0, 64, 1024, 4096, 65536):
        last = 0
        for nq in (0, 1, 2, 1023, 1024, 1025, 4096, 4097, 1 << 20, (1 << 20) + 1, N_MAX):
            need = zsfile.device_gather_scratch_bytes(nq, t)
            blocks = (nq + 1023) // 1024
            # 16 words, a sum a block of 1,024 items and one more, and for the CRC batch an offset and a length
            # an item, one 8-byte array behind the other, the whole rounded up to 16
            assert need > last and need == (8 * (16 + blocks + 1 + 2 * nq) + 15) // 16 * 16, (nq, t, need)
            last = need
    for t in (1, 32, 48, 3000, 1 << 17):
        for nq in (0, 1, 4096):
            assert zsfile.device_gather_scratch_bytes(nq, t) == 0
    assert lib().zscrc_device_gather_scratch_bytes(5, None) == zsfile.device_gather_scratch_bytes(5)
    assert zsfile.device_gather_scratch_bytes(N_MAX + 1) == 0   # above the limit on nq
    assert zsfile.device_gather_scratch_bytes(N_MAX + 1, 64) == 0
