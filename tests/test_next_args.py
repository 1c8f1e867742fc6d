"""zscrc_device_next's argument checks and its scratch size (no GPU: all of
them return before any device call), and the same checks of zscrc_zs_next."""
import ctypes

from zeroskip_amd import repack, zsfile
from zeroskip_amd._lib import lib

EINVAL = -1
PTR = 0x10000  # never dereferenced: the calls below fail their argument checks
QPTR = 0x20000
OUT = 0x80000
CUR = 0x90000
LEVELS_MAX = 64
N_MAX = (1 << 31) - 1


def _levels(*entries):
    arr = (repack.MergeList * max(len(entries), 1))()
    for j, (p, n, base) in enumerate(entries):
        arr[j].d_recs, arr[j].n, arr[j].base = p, n, base
    return arr


def _next(src=PTR, src_size=4096, levels=((PTR, 4, 0),), k=None, qsrc=QPTR, qsrc_size=64, queries=QPTR, nq=2, page=1,
          out=OUT, seq=None, cur=CUR, res=PTR, scratch=None, splitters=None, max_steps=0, flags=0):
    arr = None if levels is None else _levels(*levels)
    k = (0 if levels is None else len(levels)) if k is None else k
    opts = None if splitters is None else ctypes.byref(zsfile.NextOpts(splitters, max_steps))
    return lib().zscrc_device_next(src, src_size, arr, k, qsrc, qsrc_size, queries, nq, page, out, seq, cur, res,
                                   scratch, opts, flags, None)


def _host(src=PTR, src_size=4096, levels=((PTR, 4, 0),), k=None, qsrc=QPTR, qsrc_size=64, queries=QPTR, nq=2, page=1,
          out=OUT, seq=None, cur=CUR, res=PTR, max_steps=0, flags=0):
    arr = None if levels is None else _levels(*levels)
    k = (0 if levels is None else len(levels)) if k is None else k
    return lib().zscrc_zs_next(src, src_size, arr, k, qsrc, qsrc_size, queries, nq, page, out, seq, cur, res, max_steps,
                               flags)


# every condition the header lists, for both entries
SHARED = (dict(res=None), dict(out=None), dict(cur=None), dict(queries=None), dict(levels=None, k=1),
          dict(levels=((None, 4, 0),)), dict(levels=((PTR, 4, 0), (None, 1, 64))), dict(src=None), dict(qsrc=None),
          dict(src_size=(1 << 62) + 1), dict(qsrc_size=(1 << 62) + 1),
          dict(page=0), dict(page=65537), dict(page=(1 << 32) - 1),
          dict(nq=1 << 15, page=65536), dict(nq=N_MAX, page=2), dict(nq=(N_MAX + 1) // 2, page=2),
          dict(flags=8), dict(flags=9), dict(flags=16), dict(flags=1 << 31),
          dict(levels=((PTR, 1 << 31, 0),)), dict(levels=((PTR, N_MAX, 0), (PTR, 1, 0))),
          dict(levels=((PTR, (1 << 64) - 1, 0), (PTR, 2, 0))), dict(nq=1 << 31), dict(nq=(1 << 64) - 1),
          dict(levels=tuple((None, 0, 0) for _ in range(LEVELS_MAX + 1))))


def test_bad_arguments_are_einval():
    for bad in SHARED:
        assert _next(**bad) == EINVAL, bad
    assert _next(scratch=PTR + 8) == EINVAL               # scratch not 16-byte aligned
    assert _next(scratch=PTR + 4) == EINVAL
    for s in (3, 48, 96, 4096, 2049, 1 << 31):
        assert _next(splitters=s) == EINVAL, s
    # the largest page and the largest product pass these checks: a bad option behind them is what refuses
    assert _next(nq=(1 << 15) - 1, page=65536, splitters=3) == EINVAL


def test_the_host_form_checks_the_same_arguments():
    for bad in SHARED:
        assert _host(**bad) == EINVAL, bad


def _formula(nq, k, s):
    def up16(v):
        return (v + 15) & ~15

    each = s or zsfile.FIND_DEFAULT_SPLITTERS
    return 128 + up16(32 * (k + 1)) + (32 * each * k if each > 1 else 0) + up16(4 * nq * k)


def test_scratch_bytes_follow_the_stated_formula_and_are_monotone():
    sizes = (0, 1, 2, 3, 255, 1023, 1024, 1025, 65536, 1 << 20, N_MAX)
    for s in (0, 1, 2, 1024, 2048):
        for k in (0, 1, 4, LEVELS_MAX):
            last_q = 0
            for nq in sizes:
                need = zsfile.device_next_scratch_bytes(nq, k, s)
                assert need and need % 16 == 0 and need == _formula(nq, k, s), (nq, k, s)
                # the lookup's head and the cursors
                assert need == zsfile.device_find_scratch_bytes(k, s) + ((4 * nq * k + 15) & ~15)
                assert need >= last_q                      # monotone in nq
                last_q = need
        last_k = 0
        for k in range(LEVELS_MAX + 1):
            need = zsfile.device_next_scratch_bytes(77, k, s)
            assert need > last_k                           # monotone in k
            last_k = need
    assert zsfile.device_next_scratch_bytes(5, 2, 1) < zsfile.device_next_scratch_bytes(5, 2, 2) < \
        zsfile.device_next_scratch_bytes(5, 2, 64)


def test_scratch_bytes_are_zero_for_bad_options_and_arguments_above_their_limits():
    for s in (3, 48, 4096):
        for k in (0, 1, 64):
            assert zsfile.device_next_scratch_bytes(10, k, s) == 0
    assert zsfile.device_next_scratch_bytes(10, LEVELS_MAX + 1) == 0
    assert zsfile.device_next_scratch_bytes(N_MAX + 1, 1) == 0
    assert lib().zscrc_device_next_scratch_bytes(5, 3, None) == zsfile.device_next_scratch_bytes(5, 3)


def test_the_constants_mirror_the_header():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "zscrc.h")).read()
    for name in ("PAGE", "END", "MORE", "BAD", "INCLUSIVE", "CHECK_ORDER", "KEEP_DELETES", "RES_WORDS"):
        m = re.search(r"#define ZSCRC_NEXT_%s\s+(\d+)" % name, header)
        assert m and int(m.group(1)) == getattr(zsfile, "NEXT_" + name), name
    assert ctypes.sizeof(zsfile.NextOpts) == 8
