"""zscrc_device_merge's argument checks and its scratch size (no GPU: all of
them return before any device call)."""
import ctypes

from zeroskip_amd import repack
from zeroskip_amd._lib import lib

EINVAL = -1
PTR = 0x10000  # never dereferenced: the calls below fail their argument checks
OUT = 0x80000
WALK_MULTI_MAX = 1 << 20


def _lists(*entries):
    arr = (repack.MergeList * max(len(entries), 1))()
    for j, (p, n, base) in enumerate(entries):
        arr[j].d_recs, arr[j].n, arr[j].base = p, n, base
    return arr


def _merge(src=PTR, src_size=4096, lists=((PTR, 4, 0),), k=None, out=OUT, cap=4, res=PTR, scratch=None, tile=None,
           flags=0):
    arr = None if lists is None else _lists(*lists)
    k = (0 if lists is None else len(lists)) if k is None else k
    return lib().zscrc_device_merge(src, src_size, arr, k, out, cap, res, scratch,
                                    None if tile is None else ctypes.byref(repack.MergeOpts(tile)), flags, None)


def test_bad_arguments_are_einval():
    assert _merge(res=None) == EINVAL
    assert _merge(lists=None, k=1) == EINVAL               # k > 0 needs the lists
    assert _merge(lists=((None, 4, 0),)) == EINVAL         # n > 0 needs the records
    assert _merge(lists=((PTR, 4, 0), (None, 1, 64))) == EINVAL
    assert _merge(src=None) == EINVAL                      # src_size > 0 needs the source
    assert _merge(out=None) == EINVAL                      # cap > 0 needs the output
    assert _merge(scratch=PTR + 8) == EINVAL               # scratch not 16-byte aligned
    assert _merge(scratch=PTR + 4) == EINVAL
    for flags in (2, 3, 4, 1 << 31):
        assert _merge(flags=flags) == EINVAL, flags        # only DROP_DELETES (1) is known
    for tile in (32, 48, 96, 4096, 1, 2049, 1 << 31):
        assert _merge(tile=tile) == EINVAL, tile
    assert _merge(src_size=(1 << 62) + 1) == EINVAL        # the stated limit on src_size


def test_too_many_records_or_lists_are_einval():
    assert _merge(lists=((PTR, 1 << 31, 0),)) == EINVAL                    # n_total = 2^31
    assert _merge(lists=((PTR, (1 << 31) - 1, 0), (PTR, 1, 0))) == EINVAL  # the sum is
    assert _merge(lists=((PTR, (1 << 64) - 1, 0), (PTR, 2, 0))) == EINVAL  # a sum that would wrap
    assert _merge(lists=((PTR, 1 << 63, 0), (PTR, 1 << 63, 0))) == EINVAL
    many = (repack.MergeList * (WALK_MULTI_MAX + 1))()                     # every list empty
    assert lib().zscrc_device_merge(PTR, 4096, many, WALK_MULTI_MAX + 1, OUT, 4, PTR, None, None, 0, None) == EINVAL


def _up16(v):
    return (v + 15) // 16 * 16


def test_scratch_bytes():
    for tile in (0, 64, 256, 1024, 2048):
        last = 0
        for n in list(range(0, 40)) + [63, 64, 65, 1023, 1024, 1025, 2049, 1 << 20, (1 << 20) + 1, (1 << 21) + 3,
                                       (1 << 31) - 1]:
            need = repack.device_merge_scratch_bytes(n, tile)
            # 16 words, 24 bytes a list that is not empty and the entry that ends them, 32 + 2 x 16 bytes a record,
            # a count a block of 1,024 records and one more, a flag a record: every piece rounded up to 16
            lists, blocks = min(n, WALK_MULTI_MAX), (n + 1023) // 1024
            assert need >= last and need == 128 + _up16(24 * (lists + 1)) + 64 * n + _up16(4 * (blocks + 1)) + \
                _up16(n), (n, tile, need)
            last = need
    for tile in (32, 48, 4096):
        for n in (0, 1, 5000):
            assert repack.device_merge_scratch_bytes(n, tile) == 0
    assert lib().zscrc_device_merge_scratch_bytes(100, None) == repack.device_merge_scratch_bytes(100)
    assert repack.device_merge_scratch_bytes(1 << 31) == 0   # above the limit on n_total
