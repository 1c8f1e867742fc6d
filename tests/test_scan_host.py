"""zscrc_zs_scan, the prefix scan in host memory (one thread, no device: a
merge with one cursor a level), on every case of tests/scan_cases.py against
the dictionary model, its overflow forms, the invariants of its result words
and the reference-written repack inputs under tests/golden/ref_format.  No
GPU."""
import os

import numpy as np
import pytest

from oracle import zs_format as zf
from tests import scan_cases as sc
from tests.images import REF, UUIDSTR
from zeroskip_amd import repack, zsfile

U64 = np.uint64


def _scan(case, keep=False, check_order=False, cap=None):
    rows, offs, seqs, res = zsfile.scan(case.src, case.levels, case.qsrc, case.queries, keep_deletes=keep,
                                        check_order=check_order, cap=cap)
    return rows.view(U64), offs.view(U64), seqs.view(U64), [int(v) for v in res.view(U64)]


def _invariants(res, keep):
    assert res[0] in (0, sc.OVERFLOW) and res[10] == res[11] == 0
    if keep:
        assert res[2] + res[4] == res[3] and res[5] <= res[2]
    else:
        assert res[2] + res[4] + res[5] == res[3]


def _same(case, keep):
    rows, offs, seqs, res = _scan(case, keep)
    wrows, woffs, wseqs, wres = case.model(keep)
    assert res == wres, (case.name, keep, res, wres)
    assert rows.tobytes() == wrows.tobytes() and offs.tobytes() == woffs.tobytes() and \
        seqs.tobytes() == wseqs.tobytes(), (case.name, keep)
    _invariants(res, keep)


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in sc.small_cases()}


def test_every_small_case(cases):
    assert len(cases) >= 40
    for case in cases.values():
        for keep in (False, True):
            _same(case, keep)


def test_table_grid_and_random_cases():
    for case in sc.table_cases() + sc.random_cases():
        for keep in (False, True):
            _same(case, keep)
    for case in sc.grid_cases():
        _same(case, True)


def test_the_cases_cover_the_counts(cases):
    """C of 0 and 1 and around every size the kernels cut by; nq around the workgroup and the block."""
    assert cases["no_match"].model(False)[3][3] == 0 and cases["c1"].model(False)[3][3] == 1
    assert {c.model(True)[3][3] for c in sc.grid_cases()} == set(sc.GRID_COUNTS)
    assert sc.GRID_THREADS == zsfile.SCAN_GRID_THREADS
    assert sc.BLOCK == zsfile.SCAN_BLOCK
    for n in sc.SMALL_COUNTS:
        assert cases["c%d" % n].model(False)[3][3] == n
    assert {len(c.queries) for c in cases.values()} >= {0, 1, 63, 64, 65, 257, 1023, 1024, 1025}


def test_prefix_semantics(cases):
    """A key that is a strict prefix of the prefix is no match; keys that
    continue the prefix with zero bytes are; the empty prefix matches all."""
    c = cases["prefixes"]
    rows, offs, _, _ = _scan(c, True)
    got = {}
    for i, (off, ln) in enumerate(c.queries[:, :2].tolist()):
        got[c.qsrc[off:off + ln]] = [c.src[int(k):int(k) + int(n)] for k, n in rows[int(offs[i]):int(offs[i + 1]), :2]]
    assert got[b"abc"] == [b"abc", b"abcd"]
    assert got[b"ab"] == [b"ab", b"ab\x00", b"ab\x00\x00", b"abc", b"abcd", b"abd"]
    assert got[b"ab\x00"] == [b"ab\x00", b"ab\x00\x00"] and got[b"ab\x00\x00\x00"] == []
    assert got[b"a\xff"] == [b"a\xff", b"a\xff\xff"] and got[b"a\xff\xff"] == [b"a\xff\xff"]
    assert got[b"c\xff\xff"] == [b"c\xff\xff\x01"] and got[b"\xff"] == got[b"A"] == got[b"aa"] == got[b"zz"] == []
    assert got[b""] == sorted(set(sc.PREFIX_KEYS) | {b"bb"})


def test_winners(cases):
    c = cases["winners"]
    for keep in (False, True):
        rows, offs, seqs, res = _scan(c, keep)
        pairs = {c.src[int(k):int(k) + int(n)]: None if int(vo) == sc.U64_MAX else c.src[int(vo):int(vo) + int(vl)]
                 for k, n, vo, vl in rows[:int(offs[1])]}
        want = {b"k.every": b"0", b"k.value-over-del": b"new", b"k.zero": b"z", b"k.last": b"last"}
        if keep:
            want.update({b"k.del-over-value": None, b"k.mid": None})
        assert pairs == want and list(pairs) == sorted(pairs)


def test_row_overflow_forms(cases):
    """cap = rows - 1 and cap = 0: OVERFLOW, offs in full, exactly the rows below cap written."""
    for name in ("prefixes", "winners", "n65", "many_levels"):
        c = cases[name]
        for keep in (False, True):
            wrows, woffs, wseqs, wres = c.model(keep)
            m = len(wrows)
            assert m > 1
            for cap in (m - 1, 0):
                rows, offs, seqs, res = _scan(c, keep, cap=cap)
                assert res == [sc.OVERFLOW] + wres[1:] and res[7] == 0
                assert offs.tobytes() == woffs.tobytes()
                assert rows.tobytes() == wrows[:cap].tobytes() and seqs.tobytes() == wseqs[:cap].tobytes()
            rows, _, _, res = _scan(c, keep, cap=m + 3)
            assert res == wres and rows[:m].tobytes() == wrows.tobytes()


def test_bad_queries_are_counted_and_empty(cases):
    c = cases["bad_queries"]
    rows, offs, _, res = _scan(c)
    assert res[6] == 3 and res[0] == 0
    for i in (1, 2, 4):
        assert offs[i] == offs[i + 1]
    assert offs[1] > offs[0] and offs[4] > offs[3]


def test_a_record_outside_the_source_is_einval():
    case, seq = sc.bad_record_case()
    for check_order in (False, True):
        rows, offs, seqs, res = zsfile.scan(case.src, case.levels, case.qsrc, case.queries, check_order=check_order)
        assert [int(v) for v in res.view(U64)] == [sc.EINVAL64, seq] + [0] * 10 and len(rows) == 0


def test_check_order_offences():
    case = sc.unordered_case()
    rows, offs, seqs, res = zsfile.scan(case.src, case.levels, case.qsrc, case.queries, check_order=True)
    assert [int(v) for v in res.view(U64)] == [sc.EINVAL64, 2] + [0] * 5 + [1] + [0] * 4
    # without the check the level is scanned all the same: a result, whatever it is
    _, offs, _, res = _scan(case)
    assert res[0] == 0 and res[2] == int(offs[-1]) <= res[3]
    # a bounds offence goes before an order offence at a smaller seq
    recs = case.levels[0][0].copy()
    recs[6, 1] = len(case.src)
    both = sc.ScanCase("both", case.src, [(recs, 0), case.levels[1]], case.qsrc, case.queries)
    _, _, _, res = _scan(both, check_order=True)
    assert res[:2] == [sc.EINVAL64, 6] and res[7] == 0


def _repack_levels(name):
    """The two packed files zsdb_repack's branch 2 merges, each a level over
    one arena: (arena, newer, older, [level of 8-9, level of 4-7])."""
    d = os.path.join(REF, name)
    newer = open(os.path.join(d, "zeroskip-%s-8-9" % UUIDSTR), "rb").read()
    older = open(os.path.join(d, "zeroskip-%s-4-7" % UUIDSTR), "rb").read()
    arena = newer + bytes(-len(newer) % 64) + older
    levels = []
    for off, img in ((0, newer), (len(arena) - len(older), older)):
        recs, rc = repack.records(img, zsfile.PACKED)
        assert rc == 0
        levels.append((np.ascontiguousarray(recs.T), off))
    return arena, newer, older, levels


@pytest.mark.parametrize("name", ["repack2", "repack2d"])
def test_reference_repack_inputs(name):
    """The empty-prefix scan of the reference-written packed files.  Newest
    first, the rows are the host records sorted by the scan's rule (the model),
    deletes kept or dropped.  With the files in the order of zsdb_repack's
    priority -- branch 2 lets the OLDER file's record win (oracle/zs_format.py
    repack_packed; src/zeroskip.c:520-526) -- and deletes dropped, the rows
    are the records of the repack's default output, which the oracle's
    repack_packed states without a device (zscrc_zs_repack itself hashes on the
    GPU: tests/test_gpu_scan.py holds the scan against its output file)."""
    arena, newer, older, levels = _repack_levels(name)
    qsrc, queries = sc.fc.lay_queries([b""])
    for keep in (False, True):
        _same(sc.ScanCase(name, arena, levels, qsrc, queries), keep)
    rows, offs, _, res = zsfile.scan(arena, levels[::-1], qsrc, queries)
    got = [(arena[ko:ko + kl], arena[vo:vo + vl]) for ko, kl, vo, vl in rows.tolist()]
    assert got == zf.repack_packed(older, newer) and len(got) > 400
    assert res[4] > 0 and (res[5] > 0) == (name == "repack2d")
