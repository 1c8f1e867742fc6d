"""zscrc_device_pack's argument checks, its size bound and its scratch size (no
GPU: all of them return before any device call)."""
import ctypes

from zeroskip_amd import repack
from zeroskip_amd._lib import lib

EINVAL = -1
PTR = 0x10000  # never dereferenced: the calls below fail their argument checks
OUT = 0x80000
UUID = bytes(range(16))
U64 = 1 << 64
SHORT = 16777215


def _pack(src=PTR, src_size=4096, recs=PTR, n=4, uuid=UUID, out=OUT, cap=4096, res=PTR, scratch=None, tile=None,
          flags=0):
    return lib().zscrc_device_pack(src, src_size, recs, n, uuid, 1, 2, out, cap, res, scratch,
                                   None if tile is None else ctypes.byref(repack.PackOpts(tile)), flags, None)


def test_bad_arguments_are_einval():
    assert _pack(res=None) == EINVAL
    assert _pack(uuid=None) == EINVAL
    assert _pack(recs=None) == EINVAL                   # n > 0 needs the record list
    assert _pack(src=None) == EINVAL                    # src_size > 0 needs the source
    assert _pack(out=None) == EINVAL                    # out_cap > 0 needs the output
    assert _pack(out=OUT + 8) == EINVAL                 # output not 16-byte aligned
    assert _pack(out=OUT + 4) == EINVAL
    assert _pack(scratch=PTR + 8) == EINVAL             # scratch not 16-byte aligned
    for flags in (1, 2, 1 << 31):
        assert _pack(flags=flags) == EINVAL
    for tile in (48, 32, 1 << 17, 1, 96, (1 << 16) + 64):
        assert _pack(tile=tile) == EINVAL, tile
    assert _pack(n=1 << 31) == EINVAL                   # the stated limit on n
    assert _pack(src_size=(1 << 62) + 1) == EINVAL      # and on src_size


def test_overlapping_output_and_source_are_einval():
    for src, size, out, cap in ((0x10000, 4096, 0x10000, 4096),         # the same bytes
                                (0x10000, 4096, 0x10ff0, 4096),         # the output starts in the source's last 16
                                (0x10000, 4096, 0x0f010, 4096),         # the output ends 16 bytes into the source
                                (0x10000, 1 << 40, 0x20000, 64),        # the output inside the source
                                (0x20000, 64, 0x10000, 1 << 40)):       # the source inside the output
        assert _pack(src=src, src_size=size, out=out, cap=cap) == EINVAL, (src, size, out, cap)


def _rec(k, v):
    """Serialised length of a record: key length k, value length v (None: a delete)."""
    return 24 + ((k + 7) & ~7) + (0 if v is None else 16 + ((v + 7) & ~7))


def _exact(n, R):
    """40 + R + c(R) + 8 (n + 1) + c(8 (n + 1))."""
    def c(x):
        return 8 if x <= SHORT else 24
    return 40 + R + c(R) + 8 * (n + 1) + c(8 * (n + 1))


def test_bound_against_the_exact_size():
    assert repack.device_pack_bound(0, 0, 0) == 120 and _exact(0, 0) == 64
    for n in (1, 2, 7, 1000, 2097151, 2097152, 3000000):
        for k in (0, 1, 7, 8, 9, 65535, 65536, 70001):
            for v in (None, 0, 1, 7, 8, 9, SHORT, SHORT + 1, (16 << 20) + 9):
                # n equal records; one such record among n - 1 deletes of an empty key
                for sk, sv, R in ((k * n, (v or 0) * n, _rec(k, v) * n), (k, v or 0, _rec(k, v) + 24 * (n - 1))):
                    bound = repack.device_pack_bound(n, sk, sv)
                    assert bound == 120 + 62 * n + sk + sv and bound >= _exact(n, R), (n, k, v)


def test_bound_is_zero_on_wrap():
    for n, sk, sv in ((U64 - 1, 0, 0), (U64 // 62 + 1, 0, 0), (0, U64 - 1, 0), (0, U64 - 120, 0), (0, 0, U64 - 120),
                      (1, U64 - 182, 0), (0, 1 << 63, 1 << 63), (5, U64 - 1000, 600)):
        assert repack.device_pack_bound(n, sk, sv) == 0, (n, sk, sv)
    assert repack.device_pack_bound(0, U64 - 121, 0) == U64 - 1
    assert repack.device_pack_bound(1, U64 - 183, 0) == U64 - 1


def test_scratch_bytes():
    for tile in (0, 64, 128, 4096, 16384, 65536):
        last = 0
        for n in list(range(0, 40)) + [1023, 1024, 1025, 2047, 2048, 2049, 1 << 20, (1 << 21) + 3, (1 << 31) - 1]:
            need = repack.device_pack_scratch_bytes(n, tile)
            # 16 words, a sum a block of 1,024 records and one more, a start a record and one more, one 8-byte
            # array behind the other, the whole rounded up to 16
            blocks = (n + 1023) // 1024
            assert need >= last and need == (8 * (16 + blocks + 1 + n + 1) + 15) // 16 * 16, (n, tile, need)
            last = need
    for tile in (48, 32, 1 << 17):
        for n in (0, 1, 5000):
            assert repack.device_pack_scratch_bytes(n, tile) == 0
    assert lib().zscrc_device_pack_scratch_bytes(100, None) == repack.device_pack_scratch_bytes(100)
    assert repack.device_pack_scratch_bytes(1 << 31) == 0   # above the limit on n
