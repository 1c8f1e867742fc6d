"""zscrc_device_records_multi and zscrc_device_records_multi_scratch_bytes: what
they refuse, and what the scratch size promises (include/zscrc.h).  Every call
here returns before its first device call, so no GPU is needed: the device
pointers are made-up addresses that are never followed."""
import ctypes

import pytest

from zeroskip_amd import zsfile
from zeroskip_amd._lib import lib

EINVAL = -1
ARENA, ARENA_SIZE = 0x10000, 1 << 20      # a made-up device address; never followed
RECS, ROWS, TOT = 0x20000, 0x30000, 0x40000
U64 = (1 << 64) - 1


def _arr(images):
    return zsfile._walk_images(images)


def _list(images=((0, 4096),), arena=ARENA, arena_size=ARENA_SIZE, recs=RECS, cap=8, rows=ROWS, tot=TOT,
          scratch=None, block=0, tile=0, flags=0, k=None, null_images=False):
    arr, n = _arr(images)
    return lib().zscrc_device_records_multi(arena, arena_size, None if null_images else arr, n if k is None else k,
                                            recs, cap, rows, tot, scratch,
                                            ctypes.byref(zsfile.WalkOpts(block, tile)), flags, None)


def test_einval_is_minus_one():
    # the status the calls below are compared with is the library's own for bad arguments
    assert lib().zscrc_device_records(None, 0, zsfile.ACTIVE, None, 0, None, None, None, 0, None) == EINVAL
    assert lib().zscrc_device_records_multi(None, 0, None, 0, None, 0, None, None, None, None, 0, None) == EINVAL


def test_words():
    assert (zsfile.RECORDS_ROW_WORDS, zsfile.RECORDS_TOT_WORDS) == (12, 8)


@pytest.mark.parametrize("kw", [
    dict(arena=None),
    dict(null_images=True),
    dict(rows=None),
    dict(tot=None),
    dict(k=0),
    dict(k=zsfile.WALK_MULTI_MAX + 1),
    dict(images=[(0, 64), (ARENA_SIZE + 1, 0)]),               # off > arena_size
    dict(images=[(0, 64), (ARENA_SIZE - 8, 9)]),               # size > arena_size - off
    dict(images=[(16, U64 - 8)]),                              # off + size wraps 2^64
    dict(images=[(U64, 2)], arena_size=U64),                   # wraps, and off <= arena_size
    dict(recs=None),                                           # cap > 0 without an array
    dict(recs=None, cap=1),
    dict(flags=1),
    dict(flags=2),
    dict(scratch=0x50008),                                     # not 16-byte aligned
    dict(block=96), dict(block=32), dict(block=64, tile=128), dict(tile=32), dict(block=1 << 31),
    dict(block=1 << 20, tile=1 << 15),
    # 2^24 blocks only as the sum over the images: 64-byte blocks, 1024 images of 2^14 blocks each
    dict(images=[(0, 1 << 20)] * 1024, block=64, tile=64),
], ids=lambda kw: "-".join("%s" % k for k in kw))
def test_records_multi_refuses(kw):
    assert _list(**kw) == EINVAL


def test_limits_are_where_the_header_puts_them():
    # the neighbours of the refused cases are fine (asked of the scratch size, which makes no
    # device call either): 2^24 - 2^14 blocks in all, and images that end exactly where the arena does
    assert zsfile.records_multi_scratch_bytes([(0, 1 << 20)] * 1023 + [((1 << 20) - 64, 0)], 64, 64) > 0
    assert zsfile.records_multi_scratch_bytes([(ARENA_SIZE, 0), (ARENA_SIZE - 8, 8)]) > 0


def _bound(images, block_bytes):
    total = 64 * (len(images) + 1)
    for _, size in images:
        slots = (size + 7) // 8
        total += 8 * slots + 16 * ((slots + block_bytes // 8 - 1) // (block_bytes // 8))
    return total


def test_scratch_bytes_zero_for_bad_arguments():
    L = lib()
    opts = ctypes.byref(zsfile.WalkOpts(0, 0))
    arr, k = _arr([(0, 4096)])
    assert L.zscrc_device_records_multi_scratch_bytes(None, k, opts) == 0
    assert L.zscrc_device_records_multi_scratch_bytes(arr, 0, opts) == 0
    assert L.zscrc_device_records_multi_scratch_bytes(arr, zsfile.WALK_MULTI_MAX + 1, opts) == 0
    assert L.zscrc_device_records_multi_scratch_bytes(arr, k, None) > 0          # NULL options = defaults
    assert zsfile.records_multi_scratch_bytes([(16, U64 - 8)]) == 0
    for block, tile in ((96, 64), (32, 0), (64, 128), (0, 32), (1 << 31, 0), (1 << 20, 1 << 15)):
        assert zsfile.records_multi_scratch_bytes([(0, 4096)], block, tile) == 0, (block, tile)
    assert zsfile.records_multi_scratch_bytes([(0, 1 << 20)] * 1024, 64, 64) == 0
    assert zsfile.records_multi_scratch_bytes([(0, 1 << 30)], 64, 64) == 0       # 2^24 blocks in one image


@pytest.mark.parametrize("block,tile", [(0, 0), (64, 64), (512, 64), (4096, 512)])
def test_scratch_bytes_bound_and_growth(block, tile):
    bb = block or (1 << 20)
    sizes = [0, 1, 39, 40, 41, 47, 48, 63, 64, 65, 4095, 4096, 4097, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 3 << 20,
             100, 0, 7]
    images, last = [], 0
    for i, size in enumerate(sizes):
        images.append((i * 13, size))            # any offset: the size does not depend on it
        need = zsfile.records_multi_scratch_bytes(images, block, tile)
        assert 0 < need <= _bound(images, bb), (images, block, tile)
        assert need >= last, (images, block, tile)
        last = need
        one = zsfile.records_multi_scratch_bytes([(i * 13, size)], block, tile)
        assert 0 < one <= _bound([(0, size)], bb)
        for kind in (zsfile.ACTIVE, zsfile.FINALISED):
            assert one >= zsfile.records_scratch_bytes(size, kind, block, tile), (size, block, tile)
