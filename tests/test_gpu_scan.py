"""The device prefix scan (zscrc_device_scan, zeroskip_amd/csrc/zscrc_scan.hip)
against the dictionary model of tests/scan_cases.py and against the host scan,
at every table size.  Rows, offsets and seqs sit in canary-filled buffers
between fences: the fences always hold, on a refused call or a candidate
overflow every output byte still holds the canary, and on a row overflow
exactly the rows below cap changed."""
import os

import numpy as np
import pytest
import torch

from oracle import zs_format as zf
from tests import devmem as dm
from tests import find_cases as fc
from tests import scan_cases as sc
from tests.images import REF, U64_MAX, UUIDSTR
from zeroskip_amd import repack, zsfile

pytestmark = pytest.mark.gpu

U64 = np.uint64
SPLITS = [1, 2, 64, 2048, 0]      # no table, the smallest, a middle one, the largest, the default


def _scan(case, dev, cap, cand_cap, splitters=0, keep=False, check_order=False, scratch=None, dev_in=None):
    """device_scan into canary buffers between fences: (rows bytes [32 cap],
    offs bytes [8 (nq + 1)], seqs bytes [8 cap], res uint64 [12])."""
    d_src, levels, d_qsrc, queries = dev_in or dm.dev_in(case, dev)
    nq = int(queries.shape[0])
    wr, rows = dm.fenced(32 * cap, dev)
    wo, offs = dm.fenced(8 * (nq + 1), dev)
    ws, seqs = dm.fenced(8 * cap, dev)
    res = torch.full((zsfile.SCAN_RES_WORDS,), -6, dtype=torch.int64, device=dev)
    zsfile.device_scan(d_src, levels, d_qsrc, queries, keep_deletes=keep, check_order=check_order, cap=cap,
                       cand_cap=cand_cap, splitters=splitters,
                       out=(rows.view(torch.int64).view(cap, 4), offs.view(torch.int64), seqs.view(torch.int64), res),
                       scratch=scratch)
    return (dm.inside(wr, 32 * cap), dm.inside(wo, 8 * (nq + 1)), dm.inside(ws, 8 * cap),
            [int(v) for v in res.cpu().numpy().view(U64)])


def _same(case, dev, keeps=(False, True), splits=SPLITS, check_order=False, shift=0, qshift=0, host=True):
    """The case at every table size: equal byte for byte to the model, and the
    model to the host scan; two rows of room past the last stay untouched."""
    dev_in = dm.dev_in(case, dev, shift, qshift)
    for keep in keeps:
        wrows, woffs, wseqs, wres = case.model(keep)
        if host:
            h = zsfile.scan(case.src, case.levels, case.qsrc, case.queries, keep_deletes=keep, check_order=check_order)
            assert h[0].tobytes() == wrows.tobytes() and h[1].tobytes() == woffs.tobytes() and \
                h[2].tobytes() == wseqs.tobytes() and [int(v) for v in h[3].view(U64)] == wres, (case.name, keep)
        m = len(wrows)
        for s in splits:
            rows, offs, seqs, res = _scan(case, dev, m + 2, wres[3], s, keep, check_order, dev_in=dev_in)
            what = (case.name, keep, s, check_order, shift, qshift)
            assert res == wres, (what, res, wres)
            assert offs.tobytes() == woffs.tobytes(), what
            assert rows[:32 * m].tobytes() == wrows.tobytes() and seqs[:8 * m].tobytes() == wseqs.tobytes(), what
            assert dm.all_canary(rows[32 * m:], seqs[8 * m:]), what
        if keep:
            assert wres[2] + wres[4] == wres[3]
        else:
            assert wres[2] + wres[4] + wres[5] == wres[3]


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in sc.small_cases()}


# ----------------------------------------------------------------------- the cases
def test_structure_cases(gpu, cases):
    for name in ("no_levels", "empty_levels", "no_match", "n0", "n1", "n2", "n3", "many_levels", "twice"):
        _same(cases[name], gpu)


def test_prefix_cases(gpu, cases):
    for name in ("prefixes", "same_prefix"):
        _same(cases[name], gpu, check_order=True)


@pytest.mark.parametrize("keep", [False, True])
def test_long_prefixes(gpu, cases, keep):
    """Prefixes of 7, 8, 9, 15, 16, 17 and 70,000 bytes."""
    _same(cases["long_prefixes"], gpu, keeps=(keep,), check_order=True)


def test_winner_cases(gpu, cases):
    for name in ("winners", "deletes"):
        _same(cases[name], gpu, check_order=True)


def test_query_counts(gpu, cases):
    for nq in (0, 1, 63, 64, 65, 257, 1023, 1024, 1025):
        c = cases["nq%d" % nq]
        assert len(c.queries) == nq
        _same(c, gpu)


def test_candidate_counts_around_the_workgroup_and_the_block(gpu, cases):
    for n in sc.SMALL_COUNTS:
        c = cases["c%d" % n]
        assert c.model(False)[3][3] == n
        _same(c, gpu)


def test_candidate_counts_around_the_grid(gpu):
    """C one below, at and one above the threads of the rank's persistent grid."""
    assert sc.GRID_THREADS == zsfile.SCAN_GRID_THREADS
    for c in sc.grid_cases():
        _same(c, gpu, keeps=(True,), host=False)
        # deletes dropped: against the host scan (which test_scan_host.py holds against the model)
        got = zsfile.scan(c.src, c.levels, c.qsrc, c.queries)
        dev_in = dm.dev_in(c, gpu)
        for s in SPLITS:
            rows, offs, seqs, res = _scan(c, gpu, int(got[3][2]), int(got[3][3]), s, False, dev_in=dev_in)
            assert rows.tobytes() == got[0].tobytes() and offs.tobytes() == got[1].tobytes() and \
                seqs.tobytes() == got[2].tobytes() and res == [int(v) for v in got[3]], (c.name, s)


def test_record_counts_around_the_table_sizes(gpu, cases):
    for n in (63, 64, 65):
        _same(cases["n%d" % n], gpu)
    for c in sc.table_cases():
        _same(c, gpu)


def test_every_key_offset_and_source_address(gpu, cases):
    """residue0..7 at every table size, deletes dropped and kept; then with the
    source at shifts 1..7 and their prefix blobs at residues 0..7 shifted too,
    where only the cross product of shifts and residues is cut to two table
    sizes and one flag value."""
    for r in range(8):
        _same(cases["residue%d" % r], gpu)
        for shift in range(1, 8):
            _same(cases["residue%d" % r], gpu, keeps=(bool(shift & 1),), splits=(64, 1), shift=shift,
                  qshift=(shift * 3 + r) % 8, host=False)


@pytest.mark.parametrize("half", [0, 1])
def test_long_prefixes_at_every_source_address(gpu, cases, half):
    """The shifts of the case test_long_prefixes runs at every table size: two table sizes, deletes dropped."""
    for shift in range(1 + 4 * half, 5 + 3 * half):
        _same(cases["long_prefixes"], gpu, keeps=(False,), splits=(2, 1), shift=shift, qshift=8 - shift, host=False)


def test_bad_queries_among_good_ones(gpu, cases):
    c = cases["bad_queries"]
    assert c.model(False)[3][6] == 3
    _same(c, gpu)


def test_random_cases(gpu):
    for c in sc.random_cases():
        _same(c, gpu)


# ------------------------------------------------------------- refusals, overflows
def test_a_record_outside_the_source(gpu):
    case, seq = sc.bad_record_case()
    dev_in = dm.dev_in(case, gpu)
    for s in SPLITS:
        for check_order in (False, True):
            rows, offs, seqs, res = _scan(case, gpu, 8, 64, s, check_order=check_order, dev_in=dev_in)
            assert res == [sc.EINVAL64, seq] + [0] * 10
            assert dm.all_canary(rows, offs, seqs)


def test_check_order(gpu):
    case = sc.unordered_case()
    dev_in = dm.dev_in(case, gpu)
    for s in SPLITS:
        rows, offs, seqs, res = _scan(case, gpu, 64, 128, s, check_order=True, dev_in=dev_in)
        assert res == [sc.EINVAL64, 2] + [0] * 5 + [1] + [0] * 4
        assert dm.all_canary(rows, offs, seqs)
    # a bounds offence goes before an order offence at a smaller seq
    recs = case.levels[0][0].copy()
    recs[6, 1] = len(case.src)
    both = sc.ScanCase("both", case.src, [(recs, 0), case.levels[1]], case.qsrc, case.queries)
    for s in SPLITS:
        rows, offs, seqs, res = _scan(both, gpu, 64, 128, s, check_order=True)
        assert res == [sc.EINVAL64, 6] + [0] * 10 and dm.all_canary(rows, offs, seqs)


def test_a_level_that_does_not_ascend_stays_inside_its_buffers(gpu):
    """Without CHECK_ORDER: the rows are unspecified; the fences of the outputs
    and of the scratch hold and the code is 0."""
    for case in (sc.unordered_case(), sc.shuffled_case(0)):
        dev_in = dm.dev_in(case, gpu)
        cands = case.n * len(case.queries)         # the most there can be, whatever a bisection makes of the level
        for s in SPLITS:
            for keep in (False, True):
                need = zsfile.device_scan_scratch_bytes(len(case.queries), len(case.levels), cands, s)
                whole, scratch = dm.fenced(need, gpu)
                rows, offs, seqs, res = _scan(case, gpu, cands, cands, s, keep, scratch=scratch, dev_in=dev_in)
                assert res[0] == 0 and res[1] == len(case.queries) and res[2] <= res[3] <= cands
                dm.inside(whole, need)


def test_candidate_overflow(gpu, cases):
    """cand_cap = C - 1 against C with the repeated-prefix batch: nothing but res is written."""
    c = cases["same_prefix"]
    wrows, woffs, wseqs, wres = c.model(False)
    cands, m = wres[3], len(wrows)
    assert cands > 1000
    dev_in = dm.dev_in(c, gpu)
    for s in SPLITS:
        rows, offs, seqs, res = _scan(c, gpu, m, cands - 1, s, dev_in=dev_in)
        assert res == [sc.OVERFLOW, len(c.queries), 0, cands, 0, 0, 0, 1, 0, 0, 0, 0]
        assert dm.all_canary(rows, offs, seqs)
        rows, offs, seqs, res = _scan(c, gpu, m, cands, s, dev_in=dev_in)
        assert res == wres and rows.tobytes() == wrows.tobytes() and offs.tobytes() == woffs.tobytes()
    # the wrapper sizes itself: from the levels' records, then from the reported count
    assert cands > c.n
    rows, offs, seqs, res = zsfile.device_scan(*dev_in)
    assert [int(v) for v in res.cpu().numpy().view(U64)] == wres
    assert rows.cpu().numpy().view(U64).tobytes() == wrows.tobytes() and \
        seqs.cpu().numpy().view(U64).tobytes() == wseqs.tobytes()


def test_row_overflow(gpu, cases):
    """cap = rows - 1 and cap = 0: d_offs in full, exactly the rows below cap."""
    for name in ("prefixes", "winners", "n65", "c1025"):
        c = cases[name]
        dev_in = dm.dev_in(c, gpu)
        for keep in (False, True):
            wrows, woffs, wseqs, wres = c.model(keep)
            m = len(wrows)
            for s in SPLITS:
                rows, offs, seqs, res = _scan(c, gpu, m - 1, wres[3], s, keep, dev_in=dev_in)
                assert res == [sc.OVERFLOW] + wres[1:] and res[7] == 0, (name, res)
                assert offs.tobytes() == woffs.tobytes()
                assert rows.tobytes() == wrows[:m - 1].tobytes() and seqs.tobytes() == wseqs[:m - 1].tobytes()
        # the sizing call: cap 0, no rows buffer
        d_src, levels, d_qsrc, queries = dev_in
        offs = torch.full((len(c.queries) + 1,), -3, dtype=torch.int64, device=gpu)
        res = torch.full((zsfile.SCAN_RES_WORDS,), -6, dtype=torch.int64, device=gpu)
        zsfile.device_scan(d_src, levels, d_qsrc, queries, keep_deletes=True, cap=0, cand_cap=wres[3],
                           out=(torch.empty((0, 4), dtype=torch.int64, device=gpu), offs, None, res))
        assert [int(v) for v in res.cpu().numpy().view(U64)] == [sc.OVERFLOW] + wres[1:]
        assert offs.cpu().numpy().view(U64).tobytes() == woffs.tobytes()


# --------------------------------------------- scratch, streams and determinism
def test_caller_scratch_fenced(gpu, cases):
    for name, s in (("n65", 64), ("deletes", 2048), ("no_levels", 0), ("twice", 1), ("many_levels", 2),
                    ("c1025", 0), ("nq1025", 64)):
        c = cases[name]
        wrows, woffs, wseqs, wres = c.model(False)
        need = zsfile.device_scan_scratch_bytes(len(c.queries), len(c.levels), wres[3], s)
        assert need > 0
        whole, scratch = dm.fenced(need, gpu)
        assert scratch.data_ptr() % 16 == 0
        rows, offs, seqs, res = _scan(c, gpu, len(wrows), wres[3], s, scratch=scratch)
        assert res == wres and rows.tobytes() == wrows.tobytes() and offs.tobytes() == woffs.tobytes() and \
            seqs.tobytes() == wseqs.tobytes(), name
        dm.inside(whole, need)


def test_library_scratch_behind_a_walk_on_another_stream(gpu, cases):
    """A walk and a scan on two streams share the library's scratch, ordered by its event."""
    from tests import records_images as ri
    d_img = dm.dev_bytes(ri.wellformed(), gpu)

    def listed(walked):
        off, ln, res = (t.cpu().numpy() for t in walked)
        return off[:int(res[1])].tolist(), ln[:int(res[1])].tolist(), res.tolist()

    want_walk = listed(zsfile.device_walk(d_img))
    assert want_walk[2][1] > 0
    c = cases["n65"]
    dev_in = dm.dev_in(c, gpu)
    wrows, woffs, wseqs, wres = c.model(False)
    s1, s2 = torch.cuda.Stream(device=gpu), torch.cuda.Stream(device=gpu)
    torch.cuda.synchronize(gpu)
    for _ in range(3):
        with torch.cuda.stream(s1):
            walked = zsfile.device_walk(d_img)
        with torch.cuda.stream(s2):
            rows, offs, seqs, res = zsfile.device_scan(*dev_in, cap=len(wrows), cand_cap=wres[3], splitters=64)
        torch.cuda.synchronize(gpu)
        assert [int(v) for v in res.cpu().numpy().view(U64)] == wres
        assert rows.cpu().numpy().view(U64).tobytes() == wrows.tobytes()
        assert offs.cpu().numpy().view(U64).tobytes() == woffs.tobytes()
        assert listed(walked) == want_walk


def test_two_runs_bit_for_bit(gpu, cases):
    for c, s in ((cases["n65"], 64), (cases["many_levels"], 0), (sc.random_case(1), 2)):
        dev_in = dm.dev_in(c, gpu)
        wres = c.model(True)[3]
        a = _scan(c, gpu, wres[2], wres[3], s, True, dev_in=dev_in)
        b = _scan(c, gpu, wres[2], wres[3], s, True, dev_in=dev_in)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and a[3] == b[3] == wres


# -------------------------------------------------------------------- compositions
def _values(case, rows):
    return [None if int(vo) == U64_MAX else case.src[int(vo):int(vo) + int(vl)] for _, _, vo, vl in rows]


def test_rows_into_the_gather(gpu):
    """device_scan's rows are device_gather's items as they stand: the values equal the model's."""
    c = sc.random_case(2)
    dev_in = dm.dev_in(c, gpu)
    for keep in (False, True):
        wrows = c.model(keep)[0]
        rows, offs, seqs, res = zsfile.device_scan(*dev_in, keep_deletes=keep)
        values, voffs, crc, gres = zsfile.device_gather(dev_in[0], rows)
        v, o = values.cpu().numpy().tobytes(), voffs.cpu().numpy()
        want = _values(c, wrows)
        assert [v[int(o[i]):int(o[i + 1])] for i in range(len(wrows))] == [w or b"" for w in want]
        assert int(gres[0]) == 0 and int(gres[4]) == sum(w is None for w in want)


def test_rows_as_a_level_of_the_lookup(gpu):
    """The rows of an empty-prefix scan are a level: every row key is found at its own index."""
    c = sc.random_case(3)
    d_src, levels, _, _ = dm.dev_in(c, gpu)
    qsrc, queries = fc.lay_queries([b""])
    rows, offs, seqs, res = zsfile.device_scan(d_src, levels, dm.dev_bytes(qsrc, gpu), dm.dev_recs(queries, gpu),
                                               keep_deletes=True, check_order=True)
    n = int(res[2])
    assert n == len(rows) > 500
    hits, fres = zsfile.device_find(d_src, [(rows, 0)], d_src, rows, check_order=True)
    h = hits.cpu().numpy()
    assert int(fres[0]) == 0 and h[:, 0].tolist() == [0] * n and h[:, 1].tolist() == list(range(n))


def test_the_empty_prefix_scan_is_the_merge_reversed(gpu):
    """The merge lets the later list win, the scan the earlier level: byte for byte equal, deletes dropped or kept."""
    for c in (sc.random_case(0), sc.random_case(3), sc.winners_case(), sc.twice_case()):
        d_src, levels, _, _ = dm.dev_in(c, gpu)
        qsrc, queries = fc.lay_queries([b""])
        d_qsrc, d_q = dm.dev_bytes(qsrc, gpu), dm.dev_recs(queries, gpu)
        for keep in (False, True):
            rows, offs, seqs, res = zsfile.device_scan(d_src, levels, d_qsrc, d_q, keep_deletes=keep)
            merged, mres = repack.device_merge(d_src, levels[::-1], drop_deletes=not keep)
            assert int(res[0]) == int(mres[0]) == 0 and int(res[2]) == int(mres[1]) == len(rows)
            assert rows.cpu().numpy().tobytes() == merged.cpu().numpy().tobytes(), (c.name, keep)
            assert [int(res[i]) for i in (8, 9, 4)] == [int(mres[i]) for i in (4, 5, 6)]


def test_foreach_end_to_end(gpu):
    c = sc.winners_case()
    dev_in = dm.dev_in(c, gpu)
    wrows, woffs, _, wres = c.model(False)
    rows, offs, values, voffs, crcs, sres, gres = zsfile.device_foreach(*dev_in, crcs=True)
    assert [int(v) for v in sres.cpu().numpy().view(U64)] == wres and int(gres[0]) == 0
    assert rows.cpu().numpy().view(U64).tobytes() == wrows.tobytes()
    assert offs.cpu().numpy().view(U64).tobytes() == woffs.tobytes()
    v, o = values.cpu().numpy().tobytes(), voffs.cpu().numpy()
    got = [v[int(o[i]):int(o[i + 1])] for i in range(len(wrows))]
    assert got == _values(c, wrows)
    from oracle import oracle
    assert crcs.cpu().numpy().view(np.uint32).tolist() == [oracle.crc32c_hw(0, np.frombuffer(x, np.uint8)) if x else 0
                                                           for x in got]
    # a refused scan runs no gather
    bad, _ = sc.bad_record_case()
    out = zsfile.device_foreach(*dm.dev_in(bad, gpu))
    assert int(out[5][0]) == -1 and out[2] is None and out[6] is None


@pytest.mark.parametrize("name", ["repack2", "repack2d"])
def test_reference_repack_inputs(gpu, tmp_path, name):
    """The two packed files branch 2 of zsdb_repack merges, as levels in the
    order of its priority (the older file's record wins, src/zeroskip.c:520-526):
    the rows of the empty-prefix scan are the records of the file
    zscrc_zs_repack writes by default over a copy of the directory."""
    d = os.path.join(REF, name)
    names = ["zeroskip-%s-%s" % (UUIDSTR, r) for r in ("0-3", "4-7", "8-9")]
    for n in names:
        (tmp_path / n).write_bytes(open(os.path.join(d, n), "rb").read())
    (tmp_path / ".zsdb").write_bytes(zf.dotzsdb_bytes(4096, UUIDSTR.encode() + b"\0", 10))
    older, newer = (tmp_path / names[1]).read_bytes(), (tmp_path / names[2]).read_bytes()
    rep = repack.repack_dir(str(tmp_path))
    assert rep["branch"] == 2 and rep["files_merged"] == 2
    want = zf.packed_records(open(rep["path"], "rb").read())
    arena = older + bytes(-len(older) % 64) + newer
    d_arena = dm.dev_bytes(arena, gpu)
    levels = []
    for off, img in ((0, older), (len(arena) - len(newer), newer)):
        recs, res = zsfile.device_records(d_arena[off:off + len(img)], zsfile.PACKED)
        levels.append((recs[:int(res[1])].contiguous(), off))
    qsrc, queries = fc.lay_queries([b""])
    rows, offs, seqs, res = zsfile.device_scan(d_arena, levels, dm.dev_bytes(qsrc, gpu), dm.dev_recs(queries, gpu),
                                               check_order=True)
    got = [(arena[ko:ko + kl], arena[vo:vo + vl]) for ko, kl, vo, vl in rows.cpu().tolist()]
    assert got == want and len(got) == rep["records_out"] > 400


# -------------------------------------------------------------------------- scale
def test_more_prefixes_than_the_bounds_grid_has_threads(gpu):
    """263,144 prefixes of one or a few matches against a 1,280-record level: the
    bounds launch's grid-stride loop takes a second trip.  Against the host scan."""
    nq = zsfile.FIND_GRID_THREADS + 1000
    src, recs = fc.counted_level(1280)
    idx = np.random.default_rng(5).integers(0, 1280, nq)
    queries = recs[idx].copy()                      # the level's own records are prefixes as they stand
    queries[::3, 1] -= np.uint64(1)                 # one digit shorter: up to ten matches
    older = recs[::2].copy()
    levels = [(recs[1::3].copy(), 0), (older, 0)]
    want = zsfile.scan(src, levels, src, queries)
    wres = [int(v) for v in want[3]]
    assert wres[0] == 0 and wres[1] == nq and wres[4] > 0 and wres[5] > 0 and wres[2] > nq // 2
    assert int(want[1][-1]) > int(want[1][zsfile.FIND_GRID_THREADS]) > 0          # rows past the first trip
    d_src = dm.dev_bytes(src, gpu)
    d_levels = [(dm.dev_recs(r, gpu), b) for r, b in levels]
    d_q = dm.dev_recs(queries, gpu)
    for s in (0, 1, 2048):
        rows, offs, seqs, res = zsfile.device_scan(d_src, d_levels, d_src, d_q, cap=wres[2], cand_cap=wres[3],
                                                   splitters=s)
        assert res.cpu().numpy().tolist() == want[3].tolist(), s
        assert rows.cpu().numpy().tobytes() == want[0].tobytes() and offs.cpu().numpy().tobytes() == want[1].tobytes()
        assert seqs.cpu().numpy().tobytes() == want[2].tobytes()


def test_a_million_candidates(gpu):
    """About 2^20 candidates from 4 levels and 4,096 prefixes: trips past the grid, against the host scan."""
    n = 1 << 18
    rng = np.random.default_rng(20)
    ids = np.arange(4 * n, dtype=np.uint64)
    keys = np.sort((ids * np.uint64(0x9E3779B97F4A7C15)) & np.uint64((1 << 48) - 1))   # distinct 48-bit keys, scattered
    src = np.ascontiguousarray(keys.astype(">u8")).view(np.uint8).copy()               # as 8 big-endian bytes each
    owner = rng.integers(0, 4, 4 * n)
    levels = []
    for l in range(4):
        at = np.flatnonzero((owner == l) | (rng.integers(0, 8, 4 * n) == 0)).astype(np.uint64)
        recs = np.zeros((len(at), 4), np.uint64)
        recs[:, 0], recs[:, 1] = at * np.uint64(8) + np.uint64(2), 6                   # the six bytes that are not zero
        recs[:, 2] = np.where(at % np.uint64(7) == l, U64_MAX, at * np.uint64(8))
        recs[:, 3] = np.where(recs[:, 2] == U64_MAX, 0, 8)
        levels.append((recs, 0))
    nq = 4096
    qsrc = rng.integers(0, 256, 2 * nq, dtype=np.uint8)
    queries = np.zeros((nq, 4), np.uint64)
    queries[:, 0], queries[:, 1] = np.arange(nq, dtype=np.uint64) * np.uint64(2), 2    # two bytes: some twenty matches
    queries[::32, 1] = 1                                                               # one byte: some five thousand
    want = zsfile.scan(src, levels, qsrc, queries)
    wres = [int(v) for v in want[3]]
    assert wres[0] == 0 and wres[3] > zsfile.SCAN_GRID_THREADS * 2 and wres[4] > 0 and wres[5] > 0
    d_src, d_qsrc = dm.dev_bytes(src.tobytes(), gpu), dm.dev_bytes(qsrc.tobytes(), gpu)
    d_levels = [(dm.dev_recs(r, gpu), b) for r, b in levels]
    rows, offs, seqs, res = zsfile.device_scan(d_src, d_levels, d_qsrc, dm.dev_recs(queries, gpu), cap=wres[2],
                                               cand_cap=wres[3])
    assert res.cpu().numpy().tolist() == want[3].tolist()
    assert rows.cpu().numpy().tobytes() == want[0].tobytes() and offs.cpu().numpy().tobytes() == want[1].tobytes()
    assert seqs.cpu().numpy().tobytes() == want[2].tobytes()
