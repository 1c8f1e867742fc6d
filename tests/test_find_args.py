"""zscrc_device_find's argument checks and its scratch size (no GPU: all of
them return before any device call), and the same checks of zscrc_zs_find."""
import ctypes

from zeroskip_amd import repack, zsfile
from zeroskip_amd._lib import lib

EINVAL = -1
PTR = 0x10000  # never dereferenced: the calls below fail their argument checks
QPTR = 0x20000
OUT = 0x80000
LEVELS_MAX = 64


def _levels(*entries):
    arr = (repack.MergeList * max(len(entries), 1))()
    for j, (p, n, base) in enumerate(entries):
        arr[j].d_recs, arr[j].n, arr[j].base = p, n, base
    return arr


def _find(src=PTR, src_size=4096, levels=((PTR, 4, 0),), k=None, qsrc=QPTR, qsrc_size=64, queries=QPTR, nq=2, hits=OUT,
          res=PTR, scratch=None, splitters=None, flags=0):
    arr = None if levels is None else _levels(*levels)
    k = (0 if levels is None else len(levels)) if k is None else k
    return lib().zscrc_device_find(src, src_size, arr, k, qsrc, qsrc_size, queries, nq, hits, res, scratch,
                                   None if splitters is None else ctypes.byref(zsfile.FindOpts(splitters)), flags,
                                   None)


def test_bad_arguments_are_einval():
    assert _find(res=None) == EINVAL
    assert _find(queries=None) == EINVAL                  # nq > 0 needs the queries
    assert _find(hits=None) == EINVAL                     # and the hits
    assert _find(levels=None, k=1) == EINVAL              # k > 0 needs the levels
    assert _find(levels=((None, 4, 0),)) == EINVAL        # n > 0 needs the records
    assert _find(levels=((PTR, 4, 0), (None, 1, 64))) == EINVAL
    assert _find(src=None) == EINVAL                      # src_size > 0 needs the source
    assert _find(qsrc=None) == EINVAL                     # qsrc_size > 0 needs the query bytes
    assert _find(src_size=(1 << 62) + 1) == EINVAL        # the stated limits
    assert _find(qsrc_size=(1 << 62) + 1) == EINVAL
    assert _find(scratch=PTR + 8) == EINVAL               # scratch not 16-byte aligned
    assert _find(scratch=PTR + 4) == EINVAL
    for flags in (2, 3, 4, 1 << 31):
        assert _find(flags=flags) == EINVAL, flags        # only CHECK_ORDER (1) is known
    for s in (3, 48, 96, 4096, 2049, 1 << 31):
        assert _find(splitters=s) == EINVAL, s


def test_too_many_records_queries_or_levels_are_einval():
    assert _find(levels=((PTR, 1 << 31, 0),)) == EINVAL                    # n_total = 2^31
    assert _find(levels=((PTR, (1 << 31) - 1, 0), (PTR, 1, 0))) == EINVAL  # the sum is
    assert _find(levels=((PTR, (1 << 64) - 1, 0), (PTR, 2, 0))) == EINVAL  # a sum that would wrap
    assert _find(levels=((PTR, 1 << 63, 0), (PTR, 1 << 63, 0))) == EINVAL
    assert _find(nq=1 << 31) == EINVAL
    assert _find(nq=(1 << 64) - 1) == EINVAL
    many = (repack.MergeList * (LEVELS_MAX + 1))()                         # every level empty
    assert lib().zscrc_device_find(PTR, 4096, many, LEVELS_MAX + 1, QPTR, 64, QPTR, 2, OUT, PTR, None, None, 0,
                                   None) == EINVAL


def test_the_host_search_checks_the_same_arguments():
    def host(src=PTR, src_size=4096, levels=((PTR, 4, 0),), k=None, qsrc=QPTR, qsrc_size=64, queries=QPTR, nq=2,
             hits=OUT, res=PTR, flags=0):
        arr = None if levels is None else _levels(*levels)
        k = (0 if levels is None else len(levels)) if k is None else k
        return lib().zscrc_zs_find(src, src_size, arr, k, qsrc, qsrc_size, queries, nq, hits, res, flags)

    for bad in (dict(res=None), dict(queries=None), dict(hits=None), dict(levels=None, k=1),
                dict(levels=((None, 4, 0),)), dict(src=None), dict(qsrc=None), dict(src_size=(1 << 62) + 1),
                dict(qsrc_size=(1 << 62) + 1), dict(flags=2), dict(nq=1 << 31), dict(levels=((PTR, 1 << 31, 0),)),
                dict(levels=tuple((None, 0, 0) for _ in range(LEVELS_MAX + 1)))):
        assert host(**bad) == EINVAL, bad


def test_scratch_bytes():
    for s in (0, 1, 2, 64, 1024, 2048):
        last = 0
        for k in range(0, LEVELS_MAX + 1):
            need = zsfile.device_find_scratch_bytes(k, s)
            each = s or zsfile.FIND_DEFAULT_SPLITTERS
            table = 32 * each * k if each > 1 else 0
            # 16 words, 32 bytes a level and the entry that ends them, a table a level
            assert need > last and need == 128 + (32 * (k + 1) + 15) // 16 * 16 + table, (k, s, need)
            last = need
    for s in (3, 48, 4096):
        for k in (0, 1, 64):
            assert zsfile.device_find_scratch_bytes(k, s) == 0
    assert lib().zscrc_device_find_scratch_bytes(5, None) == zsfile.device_find_scratch_bytes(5)
    assert zsfile.device_find_scratch_bytes(LEVELS_MAX + 1) == 0   # above the limit on k
