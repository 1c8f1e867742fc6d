"""zscrc_zs_next, the successor stage in host memory (one thread, no device), on
every case of tests/next_cases.py against the dictionary model, the invariants
of its result words, its paging chain against zscrc_zs_scan, its rows against
zscrc_zs_find and the reference-written repack inputs under
tests/golden/ref_format.  No GPU."""
import os

import numpy as np
import pytest

from oracle import zs_format as zf
from tests import find_cases as fc
from tests import next_cases as nc
from tests.images import REF, UUIDSTR
from zeroskip_amd import repack, zsfile

U64 = np.uint64


def _next(case, page=1, inclusive=False, keep=False, max_steps=0, check_order=False):
    rows, seq, cur, res = zsfile.next_(case.src, case.levels, case.qsrc, case.queries, page=page, inclusive=inclusive,
                                       keep_deletes=keep, check_order=check_order, max_steps=max_steps)
    return rows.view(U64), seq.view(U64), cur.view(U64), [int(v) for v in res.view(U64)]


def invariants(res, cur, page, keep, max_steps):
    assert res[0] == 0 and res[7] == 0
    assert res[3] == (res[2] if keep else res[2] + res[5])
    states = cur[:, 3].tolist()
    assert [states.count(s) for s in (nc.PAGE, nc.END, nc.MORE, nc.BAD)] == \
        [res[1] - res[6] - res[10] - res[11], res[10], res[11], res[6]]
    assert int(cur[:, 2].sum()) == res[2] and int(cur[:, 2].max(initial=0)) <= page
    if not max_steps:
        assert res[11] == 0


def _same(case, page, inclusive, keep, max_steps):
    what = (case.name, page, inclusive, keep, max_steps)
    rows, seq, cur, res = _next(case, page, inclusive, keep, max_steps)
    wrows, wseq, wcur, wres = case.model(page, inclusive, keep, max_steps)
    assert res == wres, (what, res, wres)
    assert cur.tobytes() == wcur.tobytes(), (what, cur.tolist(), wcur.tolist())
    assert rows.tobytes() == wrows.tobytes() and seq.tobytes() == wseq.tobytes(), what
    invariants(res, cur, page, keep, max_steps)


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in nc.small_cases()}


def test_every_small_case(cases):
    assert len(cases) >= 40
    for case in cases.values():
        for setting in nc.settings(case):
            _same(case, *setting)


def test_table_and_random_cases():
    for case in nc.table_cases() + nc.random_cases():
        for setting in ((1, False, False, 0), (64, True, True, 0), (3, False, False, 2)):
            _same(case, *setting)


def test_a_thousand_deletes_and_max_steps():
    case = nc.delete_run_case(1000)
    for setting in nc.settings(case):
        _same(case, *setting)
    # the query `a` runs into the deletes: MORE until max_steps passes the run
    for steps, state, count in ((1, nc.MORE, 0), (999, nc.MORE, 0), (1000, nc.MORE, 0), (1001, nc.PAGE, 1)):
        _, _, cur, res = _next(case, 1, max_steps=steps)
        assert cur[0].tolist()[2:] == [count, state], steps


def test_the_cases_cover_the_issue_s_list(cases):
    assert {len(c.levels) for c in cases.values()} >= {0, 1, 2, 5, 64}
    assert any(len(r) == 0 for r, _ in cases["five_levels"].levels)
    assert {len(c.queries) for c in cases.values()} >= set(nc.NQ_COUNTS)
    assert {"run%d" % r for r in nc.DELETE_RUNS if r <= 65} <= set(cases)
    lens = {len(k) for k in nc.all_keys(cases["key_lengths"].src, cases["key_lengths"].levels)}
    assert lens >= set(range(0, 12)) | {17}
    assert {s[0] for c in cases.values() for s in nc.settings(c)} == set(nc.PAGES)
    assert nc.merged(cases["every_level"].src, cases["every_level"].levels)[1][b"shared"][2] == 64
    assert cases["bad_queries"].model()[3][6] == 4
    _, _, cur, res = cases["run65"].model(1, False, False, 64)
    assert res[11] >= 1 and res[5] > 0


def test_inclusive_on_a_live_a_deleted_and_an_absent_key(cases):
    c = cases["inclusive"]
    qkeys = [c.qsrc[int(o):int(o) + int(n)] for o, n in c.queries[:, :2]]

    def first_key(inclusive, keep):
        rows, _, cur, _ = _next(c, 1, inclusive, keep)
        return {q: (c.src[int(r[0, 0]):int(r[0, 0]) + int(r[0, 1])] if int(k[2]) else None)
                for q, r, k in zip(qkeys, rows, cur)}

    got = first_key(True, False)
    assert got[b"k.every"] == b"k.every" and got[b"k.zero"] == b"k.zero"          # live: the key itself
    assert got[b"k.del-over-value"] == b"k.every" and got[b"k.mid"] == b"k.value-over-del"   # deleted: the next live one
    assert got[b"k.absent"] == b"k.every" and got[b""] == b"k.every" and got[b"l"] is None
    got = first_key(False, False)
    assert got[b"k.every"] == b"k.last" and got[b"k.zero"] is None and got[b"k.value-over-del"] == b"k.zero"
    got = first_key(True, True)
    assert got[b"k.del-over-value"] == b"k.del-over-value" and got[b"k.mid"] == b"k.mid"
    got = first_key(False, True)
    assert got[b"k.del-over-value"] == b"k.every" and got[b"k.absent"] == b"k.del-over-value"


def test_filler_and_cursor_forms(cases):
    c = cases["inclusive"]
    rows, seq, cur, res = _next(c, 64)
    for i in range(len(c.queries)):
        n = int(cur[i, 2])
        assert rows[i, n:].tolist() == [list(nc.FILLER)] * (64 - n) and seq[i, n:].tolist() == [nc.U64_MAX] * (64 - n)
        assert int(cur[i, 3]) == nc.END and cur[i, :2].tolist() == [nc.NONE, 0]
    rows, seq, cur, res = _next(c, 1)
    for i in np.flatnonzero(cur[:, 3] == nc.PAGE):
        assert cur[i, :2].tolist() == rows[i, 0, :2].tolist()


# ------------------------------------------------------------------ the properties
def chain(src, levels, page, keep, max_steps=0):
    """Property (a)'s walk: from the empty key with INCLUSIVE, then the cursor
    fed back without it until the state is END: (rows, seqs, calls, MOREs seen)."""
    qsrc, queries = fc.lay_queries([b""])
    rows, seqs, calls, mores = [], [], 0, 0
    r, s, cur, res = zsfile.next_(src, levels, qsrc, queries, page=page, inclusive=True, keep_deletes=keep,
                                  max_steps=max_steps)
    while True:
        calls += 1
        n, state = int(cur[0, 2]), int(cur[0, 3])
        assert int(res[0]) == 0 and state in (nc.PAGE, nc.END, nc.MORE) and calls < 100000
        rows.append(r[0, :n])
        seqs.append(s[0, :n])
        mores += state == nc.MORE
        if state == nc.END:
            break
        r, s, cur, res = zsfile.next_(src, levels, src, cur, page=page, keep_deletes=keep, max_steps=max_steps)
    return np.concatenate(rows), np.concatenate(seqs), calls, mores


def _chain_is_the_scan(src, levels, pages=(1, 7, 64), steps=(0, 3)):
    qsrc, queries = fc.lay_queries([b""])
    for keep in (False, True):
        want = zsfile.scan(src, levels, qsrc, queries, keep_deletes=keep)
        assert int(want[3][0]) == 0
        for page in pages:
            for max_steps in steps:
                rows, seqs, calls, mores = chain(src, levels, page, keep, max_steps)
                assert rows.tobytes() == want[0].tobytes() and seqs.tobytes() == want[2].tobytes(), (page, max_steps)
                assert calls >= len(rows) // page
    return want


def test_a_chained_pages_are_the_empty_prefix_scan(cases):
    for name in ("winners", "many_levels", "five_levels", "key_lengths", "n65", "run65", "twice", "no_levels"):
        c = cases[name]
        _chain_is_the_scan(c.src, c.levels)
    c = cases["run65"]
    assert chain(c.src, c.levels, 64, False, 3)[3] > 10          # MORE occurs, and the chain goes through it
    c = nc.random_case(1)
    _chain_is_the_scan(c.src, c.levels, pages=(7, 64), steps=(0, 5))


def test_b_one_level_is_the_lookup_s_location_plus_found():
    src, recs = fc.counted_level(194)
    recs = recs[recs[:, 2] != nc.U64_MAX]                         # no deletes
    c = nc.over("live", src, [(recs, 0)])
    hits, fres = zsfile.find(c.src, c.levels, c.qsrc, c.queries)
    rows, seq, cur, res = _next(c, 1)
    assert int(fres[0]) == 0 and res[0] == 0
    for i, h in enumerate(hits.view(U64)):
        at = int(h[1]) + (int(h[0]) == 0)
        if at < len(recs):
            assert rows[i, 0].tolist() == recs[at].tolist() and int(seq[i, 0]) == at
        else:
            assert int(cur[i, 3]) == nc.END and int(cur[i, 2]) == 0


def test_c_every_row_is_where_its_seq_says(cases):
    for c in [cases[n] for n in ("many_levels", "winners", "five_levels", "shared_prefix")] + [nc.random_case(2)]:
        rows, seq, cur, res = _next(c, 3, keep=True)
        live = rows[:, :, 0] != nc.NONE
        hits, fres = zsfile.find(c.src, c.levels, c.src, rows[live])
        firsts = np.cumsum([0] + [len(r) for r, _ in c.levels])
        s = seq[live].astype(np.int64)
        level = np.searchsorted(firsts, s, side="right") - 1
        assert live.sum() > 20 and int(fres[0]) == 0
        assert hits[:, 0].tolist() == level.tolist() and hits[:, 1].tolist() == (s - firsts[level]).tolist()


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
def test_d_reference_repack_inputs(name):
    """Property (a) over the reference-written packed files with the levels in
    zsdb_repack's priority -- branch 2 lets the OLDER file's record win
    (oracle/zs_format.py repack_packed; src/zeroskip.c:520-526): the chained
    pages, deletes dropped, are the records of the repack's default output."""
    arena, newer, older, levels = _repack_levels(name)
    _chain_is_the_scan(arena, levels[::-1], pages=(7, 64), steps=(0,))
    rows, _, _, _ = chain(arena, levels[::-1], 64, False)
    got = [(arena[ko:ko + kl], arena[vo:vo + vl]) for ko, kl, vo, vl in rows.tolist()]
    assert got == zf.repack_packed(older, newer) and len(got) > 400


# ---------------------------------------------------------------------- refusals
def test_a_record_outside_the_source_is_einval():
    case, seq = nc.bad_record_case()
    for check_order in (False, True):
        rows, sq, cur, res = zsfile.next_(case.src, case.levels, case.qsrc, case.queries, page=2,
                                          check_order=check_order)
        assert [int(v) for v in res.view(U64)] == [nc.EINVAL64, seq] + [0] * 10


def test_check_order_offences():
    case = nc.unordered_case()
    _, _, _, res = _next(case, 2, check_order=True)
    assert res == [nc.EINVAL64, 2] + [0] * 5 + [1] + [0] * 4
    # without the check the level is stepped through all the same: at most n_total steps a query
    for page, keep in ((1, False), (64, True)):
        _, _, cur, res = _next(case, page, keep=keep)
        assert res[0] == 0 and res[3] <= case.n * len(case.queries)
        assert int(cur[:, 2].sum()) == res[2]
    # a bounds offence goes before an order offence at a smaller seq
    recs = case.levels[0][0].copy()
    recs[6, 1] = len(case.src)
    both = nc.NextCase("both", case.src, [(recs, 0), case.levels[1]], case.qsrc, case.queries)
    _, _, _, res = _next(both, 1, check_order=True)
    assert res[:2] == [nc.EINVAL64, 6] and res[7] == 0
