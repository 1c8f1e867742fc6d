"""zscrc_device_walk's argument checks and scratch size (no GPU: both return
before any device call)."""
import ctypes

from zeroskip_amd import zsfile
from zeroskip_amd._lib import lib

EINVAL = -1
PTR = 0x10000  # never dereferenced: the calls below fail their argument checks


def _walk(size, opts=None, flags=0, image=PTR, res=PTR, scratch=None, cap=0):
    return lib().zscrc_device_walk(image, size, None, None, cap, res, scratch,
                                   None if opts is None else ctypes.byref(zsfile.WalkOpts(*opts)), flags, None)


def test_bad_arguments_are_einval():
    assert _walk(39) == EINVAL                       # shorter than a header, as zscrc_zs_walk
    assert _walk(4096, image=None) == EINVAL
    assert _walk(4096, res=None) == EINVAL
    assert _walk(4096, cap=4) == EINVAL              # cap > 0 needs the span arrays
    assert _walk(4096, flags=2) == EINVAL            # unknown flag
    assert _walk(4096, scratch=PTR + 8) == EINVAL    # scratch not 16-byte aligned
    for opts in ((96, 64), (64, 128), (1 << 20, 32), (1 << 20, 1 << 15), (1 << 31, 64), (32, 0)):
        assert _walk(4096, opts) == EINVAL, opts
        assert zsfile.walk_scratch_bytes(4096, *opts) == 0, opts


def test_scratch_bytes_monotone_and_bounded():
    # 8 bytes per 8-byte slot and 16 per block: <= image_size + 24 * blocks
    for block, tile in ((0, 0), (64, 64), (512, 64), (4096, 512), (1 << 30, 16384)):
        bb = block or (1 << 20)
        last = 0
        for size in list(range(40, 300)) + [4095, 4096, 4097, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 5 << 30,
                                            (32 << 30) + 3]:
            need = zsfile.walk_scratch_bytes(size, block, tile)
            blocks = (size + bb - 1) // bb
            if blocks >= 1 << 24:  # more blocks than one launch has workgroups for: a bad option
                assert need == 0 and _walk(size, (block, tile)) == EINVAL, (size, block, tile)
                continue
            assert 0 < need <= size + 24 * blocks and need >= last, (size, block, tile)
            last = need
