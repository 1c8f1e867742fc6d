"""zscrc_device_log's argument checks, its size bound and its scratch size (no
GPU: all of them return before any device call), and the same checks of the
host twin zscrc_zs_log."""
import ctypes

from zeroskip_amd import zsfile
from zeroskip_amd._lib import lib

EINVAL = -1
PTR = 0x10000  # never dereferenced: the calls below fail their argument checks
OUT = 0x80000
UUID = bytes(range(16))
U64 = 1 << 64
FIN = zsfile.LOG_FINALISE


def _log(src=PTR, src_size=4096, recs=PTR, n=4, tx=PTR + 0x1000, n_tx=2, uuid=UUID, out=OUT, cap=4096, at=0,
         new_recs=None, so=None, sl=None, res=PTR, scratch=None, tile=None, flags=0):
    return lib().zscrc_device_log(src, src_size, recs, n, tx, n_tx, uuid, 1, 2, out, cap, at, new_recs, so, sl, res,
                                  scratch, None if tile is None else ctypes.byref(zsfile.LogOpts(tile, 0)), flags, None)


def _host(src=PTR, src_size=4096, recs=PTR, n=4, tx=PTR + 0x1000, n_tx=2, uuid=UUID, out=OUT, cap=4096, at=0,
          so=None, sl=None, res=PTR, tile=None, flags=0):
    return lib().zscrc_zs_log(src, src_size, recs, n, tx, n_tx, uuid, 1, 2, out, cap, at, None, so, sl, res,
                              None if tile is None else ctypes.byref(zsfile.LogOpts(tile, 0)), flags)


def test_bad_arguments_are_einval():
    for f in (_log, _host):
        assert f(res=None) == EINVAL
        assert f(uuid=None) == EINVAL                       # at == 0 writes the header
        assert f(recs=None) == EINVAL                       # n > 0 needs the record list
        assert f(tx=None) == EINVAL                         # n_tx > 0 needs the table
        assert f(src=None) == EINVAL                        # src_size > 0 needs the source
        assert f(out=None) == EINVAL                        # out_cap > 0 needs the output
        assert f(so=PTR) == EINVAL and f(sl=PTR) == EINVAL  # the span arrays come together
        for at in (1, 8, 16, 39, 41, 44, 52, 4095):
            assert f(at=at) == EINVAL, at                   # neither 0 nor a multiple of 8 from 40 up
        assert f(at=4104) == EINVAL                         # at > out_cap
        for flags in (2, 3, 4, 1 << 31):
            assert f(flags=flags) == EINVAL
        for tile in (48, 32, 1 << 17, 1, 96, (1 << 16) + 64):
            assert f(tile=tile) == EINVAL, tile
        assert f(n=1 << 31) == EINVAL                       # the stated limits
        assert f(n_tx=1 << 31) == EINVAL
        assert f(src_size=(1 << 62) + 1) == EINVAL
    assert _log(out=OUT + 8) == EINVAL                      # output not 16-byte aligned
    assert _log(out=OUT + 4) == EINVAL
    assert _log(scratch=PTR + 8) == EINVAL                  # scratch not 16-byte aligned


def test_overlap_counts_from_at():
    for f in (_log, _host):
        for src, size, out, cap, at in ((0x10000, 4096, 0x10000, 4096, 0),      # the same bytes
                                        (0x10000, 4096, 0x10ff0, 4096, 0),      # the output starts in the source
                                        (0x10000, 4096, 0x0f010, 4096, 0),      # the output ends in the source
                                        (0x10000, 1 << 40, 0x20000, 64, 0),     # the output inside the source
                                        (0x20000, 64, 0x10000, 1 << 40, 0),     # the source inside the output
                                        (0x20000, 64, 0x10000, 1 << 40, 0x10038),   # ... its last 8 bytes behind at
                                        (0x10000, 4096, 0x10000, 8192, 4088)):  # at inside the source
            assert f(src=src, src_size=size, out=out, cap=cap, at=at) == EINVAL, (src, size, out, cap, at)


def test_append_at_the_end_of_the_capacity_is_not_refused_for_its_position():
    """at == out_cap is a legal position (the call overflows on the device); with
    out_cap == 0 any legal at is the sizing call.  Only the NULL result pointer
    makes these calls return here."""
    assert _log(at=4096, res=None) == EINVAL and _host(at=4096, res=None) == EINVAL


def _exact(lens, spans):
    """40 + the records + the commits: lens (key, value or None), spans the span lengths."""
    r = sum(24 + ((k + 7) & ~7) + (0 if v is None else 16 + ((v + 7) & ~7)) for k, v in lens)
    return 40 + r + sum(8 if s <= 16777215 else 24 for s in spans)


def test_bound_against_the_exact_size():
    assert zsfile.device_log_bound(0, 0, 0, 0) == 40
    for n in (1, 2, 7, 1000):
        for k in (0, 1, 7, 8, 9, 65535, 65536):
            for v in (None, 0, 1, 7, 8, 9, 16777215, 16777216):
                lens = [(k, v)] * n
                one = _exact([(k, v)], [])- 40
                for commits, spans in ((n, [one] * n), (1, [one * n]), (n + 3, [one] * n + [0, 0, 0])):
                    b = zsfile.device_log_bound(n, commits, k * n, (v or 0) * n)
                    assert b == 40 + 54 * n + 24 * commits + k * n + (v or 0) * n and b >= _exact(lens, spans)


def test_bound_is_zero_on_wrap():
    for a in ((U64 - 1, 0, 0, 0), (U64 // 54 + 1, 0, 0, 0), (0, U64 // 24 + 1, 0, 0), (0, 0, U64 - 40, 0),
              (0, 0, 0, U64 - 40), (1, 1, U64 - 118, 0), (0, 0, 1 << 63, 1 << 63)):
        assert zsfile.device_log_bound(*a) == 0, a
    assert zsfile.device_log_bound(0, 0, U64 - 41, 0) == U64 - 1
    assert zsfile.device_log_bound(1, 1, U64 - 119, 0) == U64 - 1


def test_scratch_bytes():
    counts = list(range(0, 20)) + [1023, 1024, 1025, 2049, 1 << 20, (1 << 31) - 1]
    for tile in (0, 64, 4096, 65536):
        last_n = 0
        for n in counts:
            last_t = 0
            for t in counts:
                need = zsfile.device_log_scratch_bytes(n, t, tile)
                assert need > 0 and need % 16 == 0 and need >= last_t, (n, t)
                # 12 bytes a record, 28 a transaction, two words a block of 1,024 records, one a block of transactions
                assert need >= 12 * n + 28 * t + 16 * ((n + 1023) // 1024) + 8 * ((t + 1023) // 1024)
                assert need <= 12 * n + 28 * t + 16 * ((n + 1023) // 1024) + 8 * ((t + 1023) // 1024) + 256
                last_t = need
            assert zsfile.device_log_scratch_bytes(n, 0, tile) >= last_n       # monotone in n too
            last_n = zsfile.device_log_scratch_bytes(n, 0, tile)
    for tile in (48, 32, 1 << 17):
        assert zsfile.device_log_scratch_bytes(5, 5, tile) == 0
    assert zsfile.device_log_scratch_bytes(1 << 31, 0) == 0 and zsfile.device_log_scratch_bytes(0, 1 << 31) == 0
    assert lib().zscrc_device_log_scratch_bytes(100, 7, None) == zsfile.device_log_scratch_bytes(100, 7)
