"""zscrc_device_scan's argument checks and its scratch size (no GPU: all of
them return before any device call), and the same checks of zscrc_zs_scan."""
import ctypes

from zeroskip_amd import repack, zsfile
from zeroskip_amd._lib import lib

EINVAL = -1
PTR = 0x10000  # never dereferenced: the calls below fail their argument checks
QPTR = 0x20000
OUT = 0x80000
OFFS = 0x90000
LEVELS_MAX = 64
N_MAX = (1 << 31) - 1


def _levels(*entries):
    arr = (repack.MergeList * max(len(entries), 1))()
    for j, (p, n, base) in enumerate(entries):
        arr[j].d_recs, arr[j].n, arr[j].base = p, n, base
    return arr


def _scan(src=PTR, src_size=4096, levels=((PTR, 4, 0),), k=None, qsrc=QPTR, qsrc_size=64, queries=QPTR, nq=2, out=OUT,
          cap=8, offs=OFFS, seq=None, res=PTR, scratch=None, cand_cap=16, splitters=None, flags=0):
    arr = None if levels is None else _levels(*levels)
    k = (0 if levels is None else len(levels)) if k is None else k
    return lib().zscrc_device_scan(src, src_size, arr, k, qsrc, qsrc_size, queries, nq, out, cap, offs, seq, res,
                                   scratch, cand_cap,
                                   None if splitters is None else ctypes.byref(zsfile.ScanOpts(splitters)), flags, None)


def test_bad_arguments_are_einval():
    assert _scan(res=None) == EINVAL
    assert _scan(offs=None) == EINVAL                     # the offsets are always written
    assert _scan(out=None) == EINVAL                      # cap > 0 needs the rows
    assert _scan(queries=None) == EINVAL                  # nq > 0 needs the queries
    assert _scan(levels=None, k=1) == EINVAL              # k > 0 needs the levels
    assert _scan(levels=((None, 4, 0),)) == EINVAL        # n > 0 needs the records
    assert _scan(levels=((PTR, 4, 0), (None, 1, 64))) == EINVAL
    assert _scan(src=None) == EINVAL                      # src_size > 0 needs the source
    assert _scan(qsrc=None) == EINVAL                     # qsrc_size > 0 needs the prefix bytes
    assert _scan(src_size=(1 << 62) + 1) == EINVAL        # the stated limits
    assert _scan(qsrc_size=(1 << 62) + 1) == EINVAL
    assert _scan(scratch=PTR + 8) == EINVAL               # scratch not 16-byte aligned
    assert _scan(scratch=PTR + 4) == EINVAL
    assert _scan(cand_cap=N_MAX + 1) == EINVAL            # cand_cap above its limit
    assert _scan(cand_cap=(1 << 64) - 1) == EINVAL
    for flags in (4, 5, 8, 1 << 31):
        assert _scan(flags=flags) == EINVAL, flags        # KEEP_DELETES (1) and CHECK_ORDER (2) are known
    for s in (3, 48, 96, 4096, 2049, 1 << 31):
        assert _scan(splitters=s) == EINVAL, s


def test_too_many_records_queries_or_levels_are_einval():
    assert _scan(levels=((PTR, 1 << 31, 0),)) == EINVAL                    # n_total = 2^31
    assert _scan(levels=((PTR, N_MAX, 0), (PTR, 1, 0))) == EINVAL          # the sum is
    assert _scan(levels=((PTR, (1 << 64) - 1, 0), (PTR, 2, 0))) == EINVAL  # a sum that would wrap
    assert _scan(nq=1 << 31) == EINVAL
    assert _scan(nq=(1 << 64) - 1) == EINVAL
    many = (repack.MergeList * (LEVELS_MAX + 1))()                         # every level empty
    assert lib().zscrc_device_scan(PTR, 4096, many, LEVELS_MAX + 1, QPTR, 64, QPTR, 2, OUT, 8, OFFS, None, PTR, None,
                                   16, None, 0, None) == EINVAL


def test_the_host_scan_checks_the_same_arguments():
    def host(src=PTR, src_size=4096, levels=((PTR, 4, 0),), k=None, qsrc=QPTR, qsrc_size=64, queries=QPTR, nq=2,
             out=OUT, cap=8, offs=OFFS, seq=None, res=PTR, flags=0):
        arr = None if levels is None else _levels(*levels)
        k = (0 if levels is None else len(levels)) if k is None else k
        return lib().zscrc_zs_scan(src, src_size, arr, k, qsrc, qsrc_size, queries, nq, out, cap, offs, seq, res, flags)

    for bad in (dict(res=None), dict(offs=None), dict(out=None), dict(queries=None), dict(levels=None, k=1),
                dict(levels=((None, 4, 0),)), dict(src=None), dict(qsrc=None), dict(src_size=(1 << 62) + 1),
                dict(qsrc_size=(1 << 62) + 1), dict(flags=4), dict(nq=1 << 31), dict(levels=((PTR, 1 << 31, 0),)),
                dict(levels=tuple((None, 0, 0) for _ in range(LEVELS_MAX + 1)))):
        assert host(**bad) == EINVAL, bad


def _formula(nq, k, cand_cap, s):
    def up16(v):
        return (v + 15) & ~15

    each = s or zsfile.FIND_DEFAULT_SPLITTERS
    p = nq * k
    return 128 + up16(32 * (k + 1)) + (32 * each * k if each > 1 else 0) + up16(4 * p) + up16(8 * (p + 1)) + \
        up16(8 * (p // 1024 + 1)) + up16(4 * cand_cap) + up16(8 * (cand_cap // 1024 + 1))


def test_scratch_bytes_follow_the_stated_formula_and_are_monotone():
    sizes = (0, 1, 2, 3, 255, 1023, 1024, 1025, 65536, 1 << 20, N_MAX)
    for s in (0, 1, 2, 2048):
        for k in (0, 1, 4, LEVELS_MAX):
            last_q = 0
            for nq in sizes:
                last_c = 0
                for cand_cap in sizes:
                    need = zsfile.device_scan_scratch_bytes(nq, k, cand_cap, s)
                    assert need and need % 16 == 0 and need == _formula(nq, k, cand_cap, s), (nq, k, cand_cap, s)
                    assert need >= last_c                  # monotone in cand_cap
                    last_c = need
                    # no 32 bytes a candidate: an index and a flag
                    assert need - zsfile.device_scan_scratch_bytes(nq, k, 0, s) <= 4 * cand_cap + cand_cap // 64 + 32
                need = zsfile.device_scan_scratch_bytes(nq, k, 1000, s)
                assert need >= last_q                      # monotone in nq
                last_q = need
        last_k = 0
        for k in range(LEVELS_MAX + 1):
            need = zsfile.device_scan_scratch_bytes(77, k, 1000, s)
            assert need > last_k                           # monotone in k
            last_k = need
    assert zsfile.device_scan_scratch_bytes(5, 2, 9, 1) < zsfile.device_scan_scratch_bytes(5, 2, 9, 2) < \
        zsfile.device_scan_scratch_bytes(5, 2, 9, 64)


def test_scratch_bytes_are_zero_for_bad_options_and_arguments_above_their_limits():
    for s in (3, 48, 4096):
        for k in (0, 1, 64):
            assert zsfile.device_scan_scratch_bytes(10, k, 10, s) == 0
    assert zsfile.device_scan_scratch_bytes(10, LEVELS_MAX + 1, 10) == 0
    assert zsfile.device_scan_scratch_bytes(N_MAX + 1, 1, 10) == 0
    assert zsfile.device_scan_scratch_bytes(10, 1, N_MAX + 1) == 0
    assert lib().zscrc_device_scan_scratch_bytes(5, 3, 7, None) == zsfile.device_scan_scratch_bytes(5, 3, 7)
