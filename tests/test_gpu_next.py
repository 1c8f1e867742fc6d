"""The device successor stage (zscrc_device_next, zeroskip_amd/csrc/zscrc_next.hip)
against the dictionary model of tests/next_cases.py and against the host form,
at every table size.  Rows, seqs and cursors sit in canary-filled buffers
between fences: the fences always hold, and on a refused call every output byte
still holds the canary."""
import os

import numpy as np
import pytest
import torch

from oracle import zs_format as zf
from tests import devmem as dm
from tests import find_cases as fc
from tests import next_cases as nc
from tests.images import REF, U64_MAX, UUIDSTR
from zeroskip_amd import repack, zsfile

pytestmark = pytest.mark.gpu

U64 = np.uint64
SPLITS = [1, 2, 1024, 2048]      # no table, the smallest, the default, the largest
PLAIN = (1, False, False, 0)


def _next(case, dev, setting=PLAIN, splitters=0, check_order=False, scratch=None, dev_in=None):
    """device_next into canary buffers between fences: (rows bytes [32 nq
    page], seqs bytes [8 nq page], cur bytes [32 nq], res uint64 [12])."""
    page, inclusive, keep, max_steps = setting
    d_src, levels, d_qsrc, queries = dev_in or dm.dev_in(case, dev)
    nq = int(queries.shape[0])
    wr, rows = dm.fenced(32 * nq * page, dev)
    ws, seqs = dm.fenced(8 * nq * page, dev)
    wc, cur = dm.fenced(32 * nq, dev)
    res = torch.full((zsfile.NEXT_RES_WORDS,), -6, dtype=torch.int64, device=dev)
    zsfile.device_next(d_src, levels, d_qsrc, queries, page=page, inclusive=inclusive, keep_deletes=keep,
                       check_order=check_order, max_steps=max_steps, splitters=splitters,
                       out=(rows.view(torch.int64).view(nq, page, 4), seqs.view(torch.int64).view(nq, page),
                            cur.view(torch.int64).view(nq, 4), res), scratch=scratch)
    return (dm.inside(wr, 32 * nq * page), dm.inside(ws, 8 * nq * page), dm.inside(wc, 32 * nq),
            [int(v) for v in res.cpu().numpy().view(U64)])


def _b(a) -> bytes:
    return np.ascontiguousarray(a).tobytes()


def _equal(got, want, what):
    rows, seqs, cur, res = got
    wrows, wseqs, wcur, wres = want
    assert [int(v) for v in res] == [int(v) for v in wres], (what, res, wres)
    assert _b(cur) == _b(wcur), what
    assert _b(rows) == _b(wrows) and _b(seqs) == _b(wseqs), what


def _host(case, setting, check_order=False):
    page, inclusive, keep, max_steps = setting
    h = zsfile.next_(case.src, case.levels, case.qsrc, case.queries, page=page, inclusive=inclusive, keep_deletes=keep,
                     check_order=check_order, max_steps=max_steps)
    return h[0].view(U64), h[1].view(U64), h[2].view(U64), [int(v) for v in h[3].view(U64)]


def _same(case, dev, settings, splits=(0,), check_order=False, shift=0, qshift=0, host=True):
    """The case at every setting and table size: equal byte for byte to the
    model, and the model to the host form."""
    dev_in = dm.dev_in(case, dev, shift, qshift)
    for setting in settings:
        want = case.model(*setting)
        if host:
            _equal(_host(case, setting, check_order), want, (case.name, setting, "host"))
        for s in splits:
            _equal(_next(case, dev, setting, s, check_order, dev_in=dev_in), want,
                   (case.name, setting, s, check_order, shift, qshift))


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in nc.small_cases()}


# ----------------------------------------------------------------------- the cases
@pytest.mark.parametrize("part", range(4))
def test_every_small_case(gpu, cases, part):
    """Rows, seq, cur and res of every small case at every one of its settings."""
    names = sorted(cases)
    assert len(names) >= 40
    for name in names[part::4]:
        _same(cases[name], gpu, nc.settings(cases[name]))


@pytest.mark.parametrize("part", range(4))
def test_every_small_case_at_every_table_size(gpu, cases, part):
    for name in sorted(cases)[part::4]:
        _same(cases[name], gpu, [(1, False, False, 0), (3, True, True, 2)], SPLITS, host=False)


def test_query_counts(gpu, cases):
    for nq in nc.NQ_COUNTS:
        c = cases["nq%d" % nq]
        assert len(c.queries) == nq
        _same(c, gpu, [PLAIN, (2, True, True, 0)], [0, 1], check_order=True)


def test_one_query_more_than_the_bounds_grid_has_threads(gpu):
    """The bounds launch's grid-stride loop takes a second trip.  Against the host form."""
    nq = zsfile.FIND_GRID_THREADS + 1
    src, recs = fc.counted_level(1280)
    idx = np.random.default_rng(5).integers(0, 1280, nq)
    queries = recs[idx].copy()                      # the level's own records are queries as they stand
    queries[::3, 1] -= np.uint64(1)                 # one digit shorter: a key that is absent
    levels = [(recs[1::3].copy(), 0), (recs[::2].copy(), 0)]
    case = nc.NextCase("grid", src, levels, src, queries)
    want = _host(case, PLAIN)
    assert want[3][0] == 0 and want[3][2] > nq // 2 and want[3][5] > 0 and want[3][4] > 0
    assert int(want[2][-1, 2]) == 1                 # the query of the second trip has its row
    dev_in = dm.dev_in(case, gpu)
    for s in (0, 1):
        _equal(_next(case, gpu, PLAIN, s, dev_in=dev_in), want, ("grid", s))


def test_level_sizes_around_the_table_sizes(gpu):
    """Levels of 1 record, and of S - 1, S and S + 1 for S = 2, 1,024 and 2,048."""
    assert set(nc.LEVEL_SIZES) >= {1, 2, 3, 1023, 1024, 1025, 2047, 2048, 2049}
    for c in nc.table_cases():
        _same(c, gpu, [(2, False, False, 0), (1, True, True, 0)], SPLITS)


@pytest.mark.parametrize("shift", range(1, 8))
def test_source_and_query_address_residues(gpu, cases, shift):
    for r in range(8):
        _same(cases["residue%d" % r], gpu, [(3, bool(shift & 1), bool(shift & 2), 0)], (1024, 2), shift=shift,
              qshift=(shift * 3 + r) % 8, host=False)


def test_delete_runs_and_max_steps(gpu, cases):
    """Runs of 0 to 1,000 consecutive winning deletes after the query; max_steps at 1 and around the run."""
    for run in nc.DELETE_RUNS:
        c = cases["run%d" % run] if run <= 65 else nc.delete_run_case(run)
        extra = [s for s in nc.settings(c) if s[3]]
        assert {s[3] for s in extra} >= set(nc.run_steps(run))
        _same(c, gpu, [PLAIN, (64, False, True, 0)] + extra, [0, 1])
    _, _, cur, res = _next(nc.delete_run_case(1000), gpu, (1, False, False, 1000))
    assert cur.view(U64).reshape(-1, 4)[0].tolist()[2:] == [0, nc.MORE] and res[11] >= 1


def test_random_cases(gpu):
    for seed, c in enumerate(nc.random_cases()):
        _same(c, gpu, [PLAIN, (7, bool(seed & 1), bool(seed & 2), seed)], [0, 2, 1])


# ---------------------------------------------------------------------- refusals
def test_a_record_outside_the_source(gpu):
    case, seq = nc.bad_record_case()
    dev_in = dm.dev_in(case, gpu)
    for s in SPLITS:
        for check_order in (False, True):
            rows, seqs, cur, res = _next(case, gpu, (2, False, False, 0), s, check_order, dev_in=dev_in)
            assert res == [nc.EINVAL64, seq] + [0] * 10
            assert dm.all_canary(rows, seqs, cur)


def test_check_order(gpu):
    case = nc.unordered_case()
    dev_in = dm.dev_in(case, gpu)
    for s in SPLITS:
        rows, seqs, cur, res = _next(case, gpu, (2, True, False, 0), s, True, dev_in=dev_in)
        assert res == [nc.EINVAL64, 2] + [0] * 5 + [1] + [0] * 4
        assert dm.all_canary(rows, seqs, cur)
    # a bounds offence goes before an order offence at a smaller seq
    recs = case.levels[0][0].copy()
    recs[6, 1] = len(case.src)
    both = nc.NextCase("both", case.src, [(recs, 0), case.levels[1]], case.qsrc, case.queries)
    rows, seqs, cur, res = _next(both, gpu, PLAIN, 0, True)
    assert res == [nc.EINVAL64, 6] + [0] * 10 and dm.all_canary(rows, seqs, cur)


def test_a_level_that_does_not_ascend_stays_inside_its_buffers(gpu):
    """Without CHECK_ORDER: the rows are unspecified; the fences of the outputs
    and of the scratch hold, the code is 0 and no query takes more steps than
    there are records."""
    for case in (nc.unordered_case(), nc.shuffled_case(0)):
        dev_in = dm.dev_in(case, gpu)
        nq = len(case.queries)
        for s in SPLITS:
            for setting in ((1, False, False, 0), (64, True, True, 0)):
                need = zsfile.device_next_scratch_bytes(nq, len(case.levels), s)
                whole, scratch = dm.fenced(need, gpu)
                rows, seqs, cur, res = _next(case, gpu, setting, s, scratch=scratch, dev_in=dev_in)
                cur = cur.view(U64).reshape(-1, 4)
                assert res[0] == 0 and res[1] == nq and res[3] <= case.n * nq and int(cur[:, 2].sum()) == res[2]
                assert int(cur[:, 2].max()) <= setting[0] and set(cur[:, 3].tolist()) <= {nc.PAGE, nc.END}
                dm.inside(whole, need)


# --------------------------------------------- scratch, streams and determinism
def test_caller_scratch_fenced(gpu, cases):
    for name, s in (("n65", 64), ("deletes", 2048), ("no_levels", 0), ("twice", 1), ("many_levels", 2),
                    ("every_level", 0), ("nq257", 1024)):
        c = cases[name]
        setting = (3, True, False, 0)
        need = zsfile.device_next_scratch_bytes(len(c.queries), len(c.levels), s)
        assert need > 0
        whole, scratch = dm.fenced(need, gpu)
        assert scratch.data_ptr() % 16 == 0
        _equal(_next(c, gpu, setting, s, scratch=scratch), c.model(*setting), name)
        dm.inside(whole, need)


def test_library_scratch_behind_a_walk_on_another_stream(gpu, cases):
    """A walk and a call of the stage on two streams share the library's scratch, ordered by its event."""
    from tests import records_images as ri
    d_img = dm.dev_bytes(ri.wellformed(), gpu)

    def listed(walked):
        off, ln, res = (t.cpu().numpy() for t in walked)
        return off[:int(res[1])].tolist(), ln[:int(res[1])].tolist(), res.tolist()

    want_walk = listed(zsfile.device_walk(d_img))
    assert want_walk[2][1] > 0
    c = cases["n65"]
    dev_in = dm.dev_in(c, gpu)
    wrows, wseqs, wcur, wres = c.model(3, False, False, 0)
    s1, s2 = torch.cuda.Stream(device=gpu), torch.cuda.Stream(device=gpu)
    torch.cuda.synchronize(gpu)
    for _ in range(3):
        with torch.cuda.stream(s1):
            walked = zsfile.device_walk(d_img)
        with torch.cuda.stream(s2):
            rows, seqs, cur, res = zsfile.device_next(*dev_in, page=3, splitters=64)
        torch.cuda.synchronize(gpu)
        assert [int(v) for v in res.cpu().numpy().view(U64)] == wres
        assert rows.cpu().numpy().view(U64).tobytes() == wrows.tobytes()
        assert cur.cpu().numpy().view(U64).tobytes() == wcur.tobytes()
        assert listed(walked) == want_walk


def test_two_runs_bit_for_bit(gpu, cases):
    for c, s in ((cases["n65"], 64), (cases["many_levels"], 0), (nc.random_case(1), 2)):
        dev_in = dm.dev_in(c, gpu)
        setting = (7, False, True, 3)
        a = _next(c, gpu, setting, s, dev_in=dev_in)
        b = _next(c, gpu, setting, s, dev_in=dev_in)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and a[3] == b[3] == c.model(*setting)[3]


# ------------------------------------------------------------------ the properties
def _dev_chain(d_src, levels, dev, page, keep, max_steps=0, check_order=False):
    """Property (a)'s walk on the device: from the empty key with INCLUSIVE,
    then the cursor tensor fed back as the query list without it until the
    state is END; only the state word is read back per round.  (rows, seqs,
    calls, MOREs seen) once the chain is over."""
    qsrc, queries = fc.lay_queries([b""])
    parts, mores = [], 0
    rows, seq, cur, res = zsfile.device_next(d_src, levels, dm.dev_bytes(qsrc, dev), dm.dev_recs(queries, dev), page=page,
                                             inclusive=True, keep_deletes=keep, max_steps=max_steps,
                                             check_order=check_order)
    while True:
        parts.append((rows, seq, cur))
        state = int(cur[0, 3].cpu())
        assert state in (nc.PAGE, nc.END, nc.MORE) and len(parts) < 100000
        mores += state == nc.MORE
        if state == nc.END:
            break
        rows, seq, cur, res = zsfile.device_next(d_src, levels, d_src, cur, page=page, keep_deletes=keep,
                                                 max_steps=max_steps, check_order=check_order)
    got_rows, got_seqs = [], []
    for rows, seq, cur in parts:
        n = int(cur[0, 2].cpu())
        got_rows.append(rows[0, :n].cpu().numpy())
        got_seqs.append(seq[0, :n].cpu().numpy())
    return np.concatenate(got_rows), np.concatenate(got_seqs), len(parts), mores


def _chain_is_the_scan(src, levels, dev, pages=(1, 7, 64), steps=(0, 3)):
    qsrc, queries = fc.lay_queries([b""])
    d_src = dm.dev_bytes(src, dev)
    d_levels = [(dm.dev_recs(r, dev), b) for r, b in levels]
    for keep in (False, True):
        want = zsfile.scan(src, levels, qsrc, queries, keep_deletes=keep)
        assert int(want[3][0]) == 0
        for page in pages:
            for max_steps in steps:
                rows, seqs, calls, mores = _dev_chain(d_src, d_levels, dev, page, keep, max_steps)
                assert rows.tobytes() == want[0].tobytes() and seqs.tobytes() == want[2].tobytes(), (page, max_steps)


def test_a_chained_pages_are_the_empty_prefix_scan(gpu, cases):
    for name in ("winners", "five_levels", "n65", "no_levels"):
        _chain_is_the_scan(cases[name].src, cases[name].levels, gpu)
    _chain_is_the_scan(cases["many_levels"].src, cases["many_levels"].levels, gpu, pages=(7, 64))
    c = cases["run65"]
    _chain_is_the_scan(c.src, c.levels, gpu, pages=(1, 64))
    d_in = dm.dev_in(c, gpu)
    assert _dev_chain(d_in[0], d_in[1], gpu, 64, False, 3)[3] > 10      # MORE occurs, and the chain goes through it
    c = nc.random_case(1)
    _chain_is_the_scan(c.src, c.levels, gpu, pages=(64,), steps=(0, 50))


def test_b_one_level_is_the_lookup_s_location_plus_found(gpu):
    src, recs = fc.counted_level(194)
    recs = recs[recs[:, 2] != U64_MAX]                            # no deletes
    c = nc.over("live", src, [(recs, 0)])
    dev_in = dm.dev_in(c, gpu)
    hits, fres = zsfile.device_find(*dev_in)
    rows, seq, cur, res = zsfile.device_next(*dev_in)
    hits, rows, seq, cur = (t.cpu().numpy().view(U64) for t in (hits, rows, seq, cur))
    assert int(fres[0]) == 0 and int(res[0]) == 0
    for i, h in enumerate(hits):
        at = int(h[1]) + (int(h[0]) == 0)
        if at < len(recs):
            assert rows[i, 0].tolist() == recs[at].tolist() and int(seq[i, 0]) == at
        else:
            assert int(cur[i, 3]) == nc.END and int(cur[i, 2]) == 0


def test_c_every_row_is_where_its_seq_says(gpu, cases):
    for c in [cases[n] for n in ("many_levels", "winners", "five_levels", "shared_prefix")] + [nc.random_case(2)]:
        d_src, levels, d_qsrc, queries = dm.dev_in(c, gpu)
        rows, seq, cur, res = zsfile.device_next(d_src, levels, d_qsrc, queries, page=3, keep_deletes=True)
        live = rows[:, :, 0] != zsfile.FIND_NONE
        hits, fres = zsfile.device_find(d_src, levels, d_src, rows[live].contiguous())
        firsts = np.cumsum([0] + [len(r) for r, _ in c.levels])
        s = seq[live].cpu().numpy()
        level = np.searchsorted(firsts, s, side="right") - 1
        h = hits.cpu().numpy()
        assert len(s) > 20 and int(fres[0]) == 0
        assert h[:, 0].tolist() == level.tolist() and h[:, 1].tolist() == (s - firsts[level]).tolist()


@pytest.mark.parametrize("name", ["repack2", "repack2d"])
def test_d_reference_repack_inputs(gpu, name):
    """Property (a) over the reference-written packed files with the levels in
    zsdb_repack's priority (the older file's record wins, src/zeroskip.c:520-526):
    the chained pages, deletes dropped, are the records of the repack's output
    as oracle.zs_format.repack_packed states it."""
    d = os.path.join(REF, name)
    newer = open(os.path.join(d, "zeroskip-%s-8-9" % UUIDSTR), "rb").read()
    older = open(os.path.join(d, "zeroskip-%s-4-7" % UUIDSTR), "rb").read()
    arena = older + bytes(-len(older) % 64) + newer
    levels = []
    for off, img in ((0, older), (len(arena) - len(newer), newer)):
        recs, rc = repack.records(img, zsfile.PACKED)
        assert rc == 0
        levels.append((np.ascontiguousarray(recs.T), off))
    _chain_is_the_scan(arena, levels, gpu, pages=(7, 64), steps=(0,))
    d_levels = [(dm.dev_recs(r, gpu), b) for r, b in levels]
    rows, _, _, _ = _dev_chain(dm.dev_bytes(arena, gpu), d_levels, gpu, 64, False, check_order=True)
    got = [(arena[ko:ko + kl], arena[vo:vo + vl]) for ko, kl, vo, vl in rows.tolist()]
    assert got == zf.repack_packed(older, newer) and len(got) > 400


# -------------------------------------------------------------------- compositions
def test_fetchnext_keys_and_values(gpu, cases):
    """device_fetchnext's two CSR pairs against the bytes the model's rows name."""
    for c, keep in ((cases["winners"], False), (cases["winners"], True), (nc.random_case(3), True)):
        dev_in = dm.dev_in(c, gpu)
        wrows, wseqs, wcur, wres = c.model(3, True, keep, 0)
        keys, koffs, values, voffs, rows, seq, cur, nres, gres = zsfile.device_fetchnext(
            *dev_in, page=3, inclusive=True, keep_deletes=keep)
        assert [int(v) for v in nres.cpu().numpy().view(U64)] == wres and int(gres[0]) == 0
        assert rows.cpu().numpy().view(U64).tobytes() == wrows.tobytes()
        kb, ko = keys.cpu().numpy().tobytes(), koffs.cpu().numpy()
        vb, vo = values.cpu().numpy().tobytes(), voffs.cpu().numpy()
        flat = wrows.reshape(-1, 4).tolist()
        assert len(ko) == len(vo) == len(flat) + 1
        for r, (k_off, k_len, v_off, v_len) in enumerate(flat):
            filler = k_off == nc.NONE
            assert kb[int(ko[r]):int(ko[r + 1])] == (b"" if filler else c.src[k_off:k_off + k_len])
            live = not filler and v_off != U64_MAX
            assert vb[int(vo[r]):int(vo[r + 1])] == (c.src[v_off:v_off + v_len] if live else b"")
        assert int(gres[2]) == wres[2] - (wres[5] if keep else 0) and int(gres[5]) == sum(f[0] == nc.NONE for f in flat)
    # a refused call runs no gather
    bad, _ = nc.bad_record_case()
    out = zsfile.device_fetchnext(*dm.dev_in(bad, gpu))
    assert int(out[7][0]) == -1 and out[0] is None and out[2] is None and out[8] is None


# -------------------------------------------------------------------------- scale
def test_offsets_beyond_4_gib(gpu, cases):
    """A source of 2^32 + 64 KiB bytes whose last 64 KiB hold the keys, the
    values and the queries: every level's base, every query and every offset
    the stage writes lies above 2^32.  Against the model over that tail, the
    second call fed from the first one's cursors."""
    free, _ = torch.cuda.mem_get_info(gpu)
    if free < 6 << 30:
        pytest.skip("the source beyond 4 GiB needs 6 GiB of free device memory, %.1f GiB are free" % (free / 2**30))
    c = nc.random_case(0)
    tail = 1 << 16
    qat = (len(c.src) + 63) & ~63
    assert qat + len(c.qsrc) <= tail and len(c.levels) > 1
    size = (1 << 32) + tail
    base = 1 << 32
    d_src = torch.empty(size, dtype=torch.uint8, device=gpu)
    d_src[base:base + len(c.src)].copy_(torch.from_numpy(np.frombuffer(c.src, np.uint8).copy()))
    d_src[base + qat:base + qat + len(c.qsrc)].copy_(torch.from_numpy(np.frombuffer(c.qsrc, np.uint8).copy()))
    levels = [(dm.dev_recs(r, gpu), base + b) for r, b in c.levels]
    queries = c.queries.copy()
    queries[:, 0] += np.uint64(base + qat)

    def shifted(want):
        rows, seqs, cur = (np.array(a, dtype=U64) for a in want[:3])
        res = want[3]
        live = rows[:, :, 0] != nc.NONE
        rows[:, :, 0][live] += np.uint64(base)
        vals = live & (rows[:, :, 2] != U64_MAX)
        rows[:, :, 2][vals] += np.uint64(base)
        cur[:, 0][cur[:, 0] != nc.NONE] += np.uint64(base)
        return rows, seqs, cur, res

    setting = (3, False, True, 0)
    first = c.model(*setting)
    rows, seq, cur, res = zsfile.device_next(d_src, levels, d_src, dm.dev_recs(queries, gpu), page=3, keep_deletes=True,
                                             check_order=True)
    got = [t.cpu().numpy().view(U64) for t in (rows, seq, cur)] + [[int(v) for v in res.cpu().numpy().view(U64)]]
    _equal(got, shifted(first), "first page")
    assert int(got[0][:, :, 0][got[0][:, :, 0] != nc.NONE].min()) >= base and first[3][2] > 100
    # the second page: the cursors, all above 2^32, are the queries
    second = nc.NextCase("second", c.src, c.levels, c.src, first[2]).model(*setting)
    rows, seq, cur, res = zsfile.device_next(d_src, levels, d_src, cur, page=3, keep_deletes=True)
    got = [t.cpu().numpy().view(U64) for t in (rows, seq, cur)] + [[int(v) for v in res.cpu().numpy().view(U64)]]
    _equal(got, shifted(second), "second page")
    assert second[3][2] > 50 and second[3][6] == first[3][10] + first[3][6]
