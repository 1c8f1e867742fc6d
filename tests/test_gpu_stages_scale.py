"""The device stages with offsets, bases, outputs and files beyond 4 GiB:
zscrc_device_merge, _find, _scan, _gather, _pack, _records, _records_multi and
_walk_multi (and repack.device_repack over them) in one arena of 2^32 + 768
MiB + 77 random bytes that holds walk_images.huge_image_pieces(), two small
images behind it (both above 2^32) and the small cases of tests/huge_cases.py
at their three placements (a key byte at 2^31, at 2^32, the blob at 2^32 +
2^29 + 5).  Every expectation is a Python model's result moved by the
placement, the format oracle's packed file as pieces, numpy arithmetic or the
oracle's CRC over the host copy of the arena; the host twins are compared in
addition.  Every test asserts on its own inputs that they cross what it is
there to cross, and prints its wall time."""
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import oracle
from tests import gather_cases as gc
from tests import huge_cases as hc
from tests import records_images as ri
from tests import walk_images as wi
from tests.arena_cases import first_unaligned as _first_unaligned
from tests.arena_cases import records_check as _records_check
from tests.arena_cases import records_run as _records_run
from tests.arena_cases import trajectory as _trajectory
from tests.arena_cases import walk_check as _walk_check
from tests.arena_cases import walk_run as _walk_run
from tests.devmem import CANARY, PAD
from tests.devmem import dev_recs as _dev_recs
from tests.devmem import fenced as _fenced
from tests.devmem import inside as _inside
from tests.images import UUID
from tests.records_images import folds as _folds
from zeroskip_amd import repack, zsfile
from zeroskip_amd._lib import lib

pytestmark = pytest.mark.gpu

U64 = np.uint64
B31, B32 = hc.B31, hc.B32
MIB = 1 << 20
A, F, P = zsfile.ACTIVE, zsfile.FINALISED, zsfile.PACKED
HUGE_VALUE = (37, B32 + 5 * MIB + 3)         # (val_off, val_len) of the gather's and the packer's huge record
MEDIUM = MIB + 1
LIST_CAP = 8192                              # more records than any image here holds


def _dev_lists(lists, dev) -> list:
    return [(_dev_recs(r, dev), b) for r, b in lists]


def _canary_on_device(t: torch.Tensor) -> bool:
    return bool((t == CANARY).all())


def _words(a) -> list:
    return [int(v) for v in np.asarray(a).view(U64).ravel()]


def _top(lists) -> int:
    """The largest key offset of [(recs, base)], base added."""
    return max(int(r[:, 0].max()) + int(b) for r, b in lists if len(r))


# ------------------------------------------------------------------ the arena
@pytest.fixture(scope="module")
def big(gpu):
    free, _ = torch.cuda.mem_get_info(gpu)
    if free < 24 << 30:
        pytest.skip("the arena beyond 4 GiB, its outputs and the library's scratch need 24 GiB of free device memory, "
                    "%.1f GiB are free" % (free / 2 ** 30))
    t0 = time.perf_counter()
    w = hc.world()
    g = torch.Generator(device=gpu)
    g.manual_seed(2026)
    d = torch.randint(0, 256, (hc.ARENA_BYTES,), dtype=torch.uint8, device=gpu, generator=g)

    def put(off, b):
        d[off:off + len(b)] = torch.from_numpy(np.ascontiguousarray(b).copy()).to(gpu)

    # 1. the huge image at 0 (its value body stays random)  2. two small images behind it  3. the small blobs
    pieces, huge_size = wi.huge_image_pieces()
    for at, b in pieces:
        put(at, np.frombuffer(b, np.uint8))
    images, at = [(0, huge_size)], huge_size
    small = [ri.wellformed(), ri.finalised_300()]
    for img in small:
        at = (at + 7) & ~7
        put(at, np.frombuffer(img, np.uint8))
        images.append((at, len(img)))
        at += len(img)
    body = pieces[1][0] + len(pieces[1][1])                    # the huge value's body: blobs may lie in it
    lay = w.layout
    lay.check(reserved=[(0, body), (body + wi.HUGE_VALUE, at - body - wi.HUGE_VALUE)])
    assert images[1][0] > B32 and images[2][0] > B32 and images[1][0] % 8 == 0 and images[2][0] % 8 == 0
    lay.fill(put)
    torch.cuda.synchronize(gpu)
    h = d.cpu().numpy()                                        # the one copy every reference reads
    # per image: the host lister's records and the host walk, image-relative
    lists, walks = [], []
    for off, size in images:
        img = h[off:off + size]
        recs, rc, n = ri.host_records_capped(img, A, LIST_CAP)
        assert rc == zsfile.END and n == len(recs) < LIST_CAP
        lists.append(recs)
        walks.append(wi.host_walk_capped(img, LIST_CAP))
    assert int(lists[0][:, 3].max()) == wi.HUGE_VALUE > B32 and int(lists[0][:, 0].max()) > B32
    # the two long CRCs the expected packed files chain through (eight threads, kept by huge_cases)
    hc.span_crc(h, *HUGE_VALUE)
    hc.span_crc(h, body, wi.HUGE_VALUE)
    s = SimpleNamespace(w=w, d=d, h=h, images=images, small=small, lists=lists, walks=walks, dev=gpu)
    print(f"arena beyond 4 GiB built, copied and listed: {time.perf_counter() - t0:.2f} s")
    yield s
    del s.d, d
    torch.cuda.empty_cache()
    lib().zscrc_release_cache()


# ------------------------------------------------------------------ a. merge
def _merge(d_src, lists, drop, cap, tile):
    whole, out = _fenced(32 * cap, d_src.device)
    _, res = repack.device_merge(d_src, lists, drop_deletes=drop, out=out.view(torch.int64).view(cap, 4),
                                 tile_records=tile)
    return _inside(whole, 32 * cap).view(U64).reshape(cap, 4), _words(res.cpu().numpy())


def _merged_equal(got, want, wres, what):
    rows, res = got
    assert res == wres, (what, res, wres)
    assert rows[:len(want)].tolist() == want.tolist(), what
    assert bool((rows[len(want):].view(np.uint8) == CANARY).all()), what


def test_merge_beyond_4gib(big):
    t0 = time.perf_counter()
    above = 0
    for c, p in big.w.merge:
        d_src = p.view(big.d)
        models = {drop: c.model(drop) for drop in (False, True)}
        for place in hc.PLACES:
            for carry in hc.CARRIES:
                lists = hc.carried(c.lists, p.P[place], carry)
                hc.expect_crossing(lists, place, c.name)
                above += _top(lists) > B32
                d_lists = _dev_lists(lists, big.dev)
                for drop in (False, True):
                    want, wres = models[drop]
                    want = hc.shift_recs(want, p.P[place])
                    for tile in (64, 0):
                        _merged_equal(_merge(d_src, d_lists, drop, len(want) + 3, tile), want, wres,
                                      (c.name, place, carry, drop, tile))
        # the lists in turn at two placements of the blob, each with its own base
        for a, b in (("at_2g", "odd"), ("at_4g", "at_2g")):
            for drop in (False, True):
                lists, want, wres = hc.two_places(c, p, a, b, drop)
                assert {int(base) for _, base in lists} <= {p.P[a], p.P[b]}
                _merged_equal(_merge(d_src, _dev_lists(lists, big.dev), drop, len(want) + 3, 0), want, wres,
                              (c.name, a, b, drop))
                if len(c.lists) > 1 and b == "odd":         # winners of lists on both sides of 2^32
                    ko = want[:, 0]
                    assert bool((ko > U64(B32)).any()) and bool((ko < U64(B32)).any()), c.name
    assert above >= 2 * len(big.w.merge)
    print(f"merge beyond 4 GiB: {time.perf_counter() - t0:.2f} s")


# ------------------------------------------------------------------ b. find
def _find(d_src, levels, d_qsrc, queries, splitters):
    nq = int(queries.shape[0])
    whole, out = _fenced(32 * nq, d_src.device)
    res = torch.full((8,), -6, dtype=torch.int64, device=d_src.device)
    zsfile.device_find(d_src, levels, d_qsrc, queries, splitters=splitters, out=(out.view(torch.int64).view(nq, 4), res))
    return _inside(whole, 32 * nq).view(U64).reshape(nq, 4), _words(res.cpu().numpy())


def test_find_beyond_4gib(big):
    t0 = time.perf_counter()
    straddlers = 0
    for c, p, qp in big.w.find:
        want, wres = c.model()
        d_src, d_qsrc = p.view(big.d), qp.view(big.d)
        h_src, h_qsrc = p.view(big.h), qp.view(big.h)
        for place in hc.PLACES:
            queries = hc.shift_queries(c.queries, qp.P[place])
            hc.expect_crossing([(queries, 0)], place, c.name)
            q = queries[:, 0].astype(object)
            straddlers += place == "at_4g" and bool(((q < B32) & (q + queries[:, 1].astype(object) > B32)).any())
            d_queries = _dev_recs(queries, big.dev)
            shifted = hc.shift_hits(want, p.P[place])
            for carry in hc.CARRIES:
                levels = hc.carried(c.levels, p.P[place], carry)
                hc.expect_crossing(levels, place, c.name)
                assert place != "odd" or (_top(levels) > B32 and int(queries[:, 0].min()) > B32)
                what = (c.name, place, carry)
                hh, hres = zsfile.find(h_src, levels, h_qsrc, queries)
                assert _words(hres) == wres and hh.view(U64).tobytes() == shifted.tobytes(), what
                d_levels = _dev_lists(levels, big.dev)
                for s in (1, 0):
                    hits, res = _find(d_src, d_levels, d_qsrc, d_queries, s)
                    assert res == wres, (what, s, res, wres)
                    assert hits.tobytes() == shifted.tobytes(), (what, s, np.argwhere(hits != shifted)[:4].tolist())
    assert straddlers >= 3          # query keys with bytes on both sides of 2^32
    print(f"find beyond 4 GiB: {time.perf_counter() - t0:.2f} s")


# ------------------------------------------------------------------ c. scan
def _scan(d_src, levels, d_qsrc, queries, cap, cand_cap, splitters, keep):
    dev, nq = d_src.device, int(queries.shape[0])
    wr, rows = _fenced(32 * cap, dev)
    wo, offs = _fenced(8 * (nq + 1), dev)
    ws, seqs = _fenced(8 * cap, dev)
    res = torch.full((zsfile.SCAN_RES_WORDS,), -6, dtype=torch.int64, device=dev)
    zsfile.device_scan(d_src, levels, d_qsrc, queries, keep_deletes=keep, cap=cap, cand_cap=cand_cap,
                       splitters=splitters,
                       out=(rows.view(torch.int64).view(cap, 4), offs.view(torch.int64), seqs.view(torch.int64), res))
    return _inside(wr, 32 * cap), _inside(wo, 8 * (nq + 1)), _inside(ws, 8 * cap), _words(res.cpu().numpy())


def test_scan_beyond_4gib(big):
    t0 = time.perf_counter()
    for c, p, qp in big.w.scan:
        d_src, d_qsrc = p.view(big.d), qp.view(big.d)
        h_src, h_qsrc = p.view(big.h), qp.view(big.h)
        for place in hc.PLACES:
            queries = hc.shift_queries(c.queries, qp.P[place])
            hc.expect_crossing([(queries, 0)], place, c.name)
            d_queries = _dev_recs(queries, big.dev)
            for carry in hc.CARRIES:
                levels = hc.carried(c.levels, p.P[place], carry)
                hc.expect_crossing(levels, place, c.name)
                assert place != "odd" or (_top(levels) > B32 and int(queries[:, 0].min()) > B32)
                d_levels = _dev_lists(levels, big.dev)
                for keep in (False, True):
                    wrows, woffs, wseqs, wres = c.model(keep)
                    wrows = hc.shift_recs(wrows, p.P[place])
                    m = len(wrows)
                    assert place != "odd" or m == 0 or int(wrows[:, 0].min()) > B32
                    what = (c.name, place, carry, keep)
                    hr = zsfile.scan(h_src, levels, h_qsrc, queries, keep_deletes=keep)
                    assert hr[0].view(U64).tobytes() == wrows.tobytes() and hr[1].view(U64).tobytes() == woffs.tobytes() \
                        and hr[2].view(U64).tobytes() == wseqs.tobytes() and _words(hr[3]) == wres, what
                    for s in (1, 0):
                        rows, offs, seqs, res = _scan(d_src, d_levels, d_qsrc, d_queries, m + 2, wres[3], s, keep)
                        assert res == wres, (what, s, res, wres)
                        assert offs.tobytes() == woffs.tobytes(), (what, s)
                        assert rows[:32 * m].tobytes() == wrows.tobytes(), (what, s)
                        assert seqs[:8 * m].tobytes() == wseqs.tobytes(), (what, s)
                        assert bool((rows[32 * m:] == CANARY).all() and (seqs[8 * m:] == CANARY).all()), (what, s)
    print(f"scan beyond 4 GiB: {time.perf_counter() - t0:.2f} s")


# ------------------------------------------------------------------ d. gather, small outputs
def _gather(d_src, d_items, cap, tile):
    dev, nq = d_src.device, int(d_items.shape[0])
    w_out, out = _fenced(cap, dev)
    w_offs, offs = _fenced(8 * (nq + 1), dev)
    w_crc, crc = _fenced(4 * nq, dev)
    res = torch.full((8,), -6, dtype=torch.int64, device=dev)
    zsfile.device_gather(d_src, d_items, cap=cap, tile_bytes=tile,
                         out=(out, offs.view(torch.int64), crc.view(torch.int32), res))
    return (_inside(w_out, cap), _inside(w_offs, 8 * (nq + 1)).view(U64), _inside(w_crc, 4 * nq).view(np.uint32),
            _words(res.cpu().numpy()))


def _gathered_equal(big, p, items, want, what):
    values, offs, crcs, res = want
    total = res[3]
    hv, ho, hcrc, hr = zsfile.gather(p.view(big.h), items, crcs=True)
    assert _words(hr) == res and hv.tobytes() == values.tobytes() and ho.view(U64).tobytes() == offs.tobytes(), what
    assert hcrc.tobytes() == crcs.tobytes(), what
    d_items = _dev_recs(items, big.dev)
    for tile in (64, 0):
        out, o, c, r = _gather(p.view(big.d), d_items, total + 48, tile)
        assert r == res, (what, tile, r, res)
        assert o.tobytes() == offs.tobytes(), (what, tile)
        assert out[:total].tobytes() == values.tobytes(), (what, tile, np.flatnonzero(out[:total] != values)[:4].tolist())
        assert bool((out[total:] == CANARY).all()), (what, tile)
        assert c.tobytes() == crcs.tobytes(), (what, tile)


def test_gather_small_outputs_beyond_4gib(big):
    t0 = time.perf_counter()
    for c, p in big.w.gather:
        want = c.model()
        o = want[1].tolist()
        assert want[2].tolist() == [oracle.crc32c_hw(0, want[0][o[i]:o[i + 1]]) if o[i + 1] > o[i] else 0
                                    for i in range(c.nq)]
        for place in hc.PLACES:
            items = hc.shift_items(c.items, p.P[place])
            val = items[gc.kinds(items)[0]]
            assert int((val[:, 2] + val[:, 3]).max()) > (B31 if place == "at_2g" else B32), (c.name, place)
            assert place != "odd" or int(val[:, 2].min()) > B32
            _gathered_equal(big, p, items, want, (c.name, place))
    # the hits of a lookup beyond 4 GiB, as the find leaves them
    for c, p, qp in big.w.find:
        hits, _ = c.model()
        want = gc.model(c.src, hits)
        for place in ("at_4g", "odd"):
            items = hc.shift_hits(hits, p.P[place])
            found = items[gc.kinds(items)[0]]
            assert len(found) and (place != "odd" or int(found[:, 2].min()) > B32), c.name
            _gathered_equal(big, p, items, want, (c.name, place, "hits"))
    print(f"gather of small outputs beyond 4 GiB: {time.perf_counter() - t0:.2f} s")


# ------------------------------------------------------------------ e. gather, outputs beyond 4 GiB
def _huge_items(shape: str) -> np.ndarray:
    if shape == "one_huge":
        # a small value, the huge one, a miss, a delete, 1 MiB + 1 from an odd offset, a small value across 2^31
        return gc.items_of([gc.value(B32 + 12_345, 100), gc.value(*HUGE_VALUE), gc.MISS, gc.DELETE,
                            gc.value(B32 + 600 * MIB + 1, MEDIUM), gc.value(B31 - 7, 29)])
    return gc.items_of([gc.value(B32 + 300 * MIB + 7, MEDIUM)] * 4200)


@pytest.fixture(scope="module")
def huge_gathers(big):
    """shape -> (items, offs, the eight result words, the oracle's CRCs): numpy and the oracle over the host copy."""
    t0 = time.perf_counter()
    out = {}
    for shape in ("one_huge", "many_medium"):
        items = _huge_items(shape)
        val = gc.kinds(items)[0]
        lens = np.where(val, items[:, 3], U64(0))
        offs = np.zeros(len(items) + 1, U64)
        np.cumsum(lens, out=offs[1:])
        assert int((items[val, 2] + items[val, 3]).max()) <= big.h.size
        crcs = oracle.batch(big.h, np.where(val, items[:, 2], U64(0)), lens, impl="hw", threads=8)
        crcs[lens == 0] = 0
        kinds = gc.kinds(items)
        res = [0, len(items), int(val.sum()), int(offs[-1]), int(kinds[1].sum()), int(kinds[2].sum()),
               int(kinds[3].sum()), int(lens.max())]
        assert res[3] > B32 and bool((offs[1:-1] < U64(B32)).any()) and bool((offs[1:-1] > U64(B32)).any())
        out[shape] = (items, offs, res, crcs)
    assert int(out["one_huge"][0][1, 3]) > B32 and int(out["many_medium"][0][0, 2]) % 2 == 1
    last = out["one_huge"][0][5]
    assert int(last[2]) < B31 < int(last[2] + last[3]) and int(out["one_huge"][0][4, 2]) % 2 == 1
    print(f"references of the gathers beyond 4 GiB: {time.perf_counter() - t0:.2f} s")
    return out


@pytest.mark.parametrize("tile", [0, 65536], ids=["default", "t65536"])
@pytest.mark.parametrize("shape", ["one_huge", "many_medium"])
def test_gather_outputs_beyond_4gib(big, huge_gathers, shape, tile):
    t0 = time.perf_counter()
    items, offs, wres, wcrcs = huge_gathers[shape]
    nq, total, dev = len(items), wres[3], big.dev
    cap = total + 48
    whole, out = _fenced(cap, dev)
    w_offs, d_offs = _fenced(8 * (nq + 1), dev)
    w_crc, d_crc = _fenced(4 * nq, dev)
    res = torch.full((8,), -6, dtype=torch.int64, device=dev)
    zsfile.device_gather(big.d, _dev_recs(items, dev), cap=cap, tile_bytes=tile,
                         out=(out, d_offs.view(torch.int64), d_crc.view(torch.int32), res))
    assert _words(res.cpu().numpy()) == wres
    assert _inside(w_offs, 8 * (nq + 1)).tobytes() == offs.tobytes()
    assert _inside(w_crc, 4 * nq).view(np.uint32).tolist() == wcrcs.tolist()
    o = offs.tolist()
    if shape == "one_huge":
        for i, (_, _, vo, vl) in enumerate(items.tolist()):
            if o[i + 1] > o[i]:
                assert torch.equal(out[o[i]:o[i + 1]], big.d[vo:vo + vl]), i
    else:
        vo, vl = int(items[0, 2]), int(items[0, 3])
        src = big.d[vo:vo + vl]
        for i in range(0, nq, 300):
            k = min(300, nq - i)
            assert bool((out[o[i]:o[i + k]].view(k, vl) == src).all()), i
    # the 48 + 4,096 bytes behind the total, and the fence in front
    assert _canary_on_device(whole[PAD + total:]) and _canary_on_device(whole[:PAD])
    print(f"gather beyond 4 GiB ({shape}, tile {tile}): {time.perf_counter() - t0:.2f} s")


def test_gather_overflow_beyond_4gib(big, huge_gathers):
    """cap = total - 1: code 3, the offsets complete, no value byte and every CRC 0."""
    t0 = time.perf_counter()
    items, offs, wres, _ = huge_gathers["one_huge"]
    nq, total, dev = len(items), wres[3], big.dev
    assert total - 1 > B32
    whole, out = _fenced(total - 1, dev)
    w_offs, d_offs = _fenced(8 * (nq + 1), dev)
    w_crc, d_crc = _fenced(4 * nq, dev)
    res = torch.full((8,), -6, dtype=torch.int64, device=dev)
    zsfile.device_gather(big.d, _dev_recs(items, dev), cap=total - 1, out=(out, d_offs.view(torch.int64),
                                                                           d_crc.view(torch.int32), res))
    assert _words(res.cpu().numpy()) == [gc.OVERFLOW] + wres[1:]
    assert _inside(w_offs, 8 * (nq + 1)).tobytes() == offs.tobytes()
    assert _inside(w_crc, 4 * nq).view(np.uint32).tolist() == [0] * nq
    assert _canary_on_device(whole)
    print(f"gather overflow beyond 4 GiB: {time.perf_counter() - t0:.2f} s")


# ------------------------------------------------------------------ f. pack
def _packed_equal(big, out, exp, what):
    """The written image against the pieces, the lister and the verifier."""
    for at, b in exp.runs:
        got = out[at:at + len(b)].cpu().numpy().tobytes()
        assert got == b, (what, at, len(b), next(i for i in range(len(b)) if got[i] != b[i]))
    for at, src, n in exp.bodies:
        assert torch.equal(out[at:at + n], big.d[src:src + n]), (what, at, src, n)
    n = len(exp.recs)
    fr, recs = _fenced(32 * (n + 8), big.dev)
    _, lres = zsfile.device_records(out[:exp.file_bytes], P, cap=n + 8,
                                    out=(recs.view(torch.int64).view(n + 8, 4),
                                         torch.empty(zsfile.RECORDS_RES_WORDS, dtype=torch.int64, device=big.dev)))
    lr = _words(lres.cpu().numpy())
    listed = _inside(fr, 32 * (n + 8)).view(U64).reshape(n + 8, 4)
    assert lr[:3] == [0, n, exp.pointers_at], (what, lr)
    assert np.array_equal(listed[:n], exp.recs), what
    v = zsfile.verify_device_image(out[:exp.file_bytes], P)
    assert (v["header_rc"], v["walk_rc"], v["n_commits"], v["n_bad"]) == (0, 0, 2, 0), (what, v)
    assert v["header_stored"] == v["header_computed"], what


def test_pack_file_beyond_4gib(big):
    t0 = time.perf_counter()
    w = big.w
    # record-carried: the first half of the list reads the blob's copy in [2^31, 2^32), the second half the one above 2^32
    mid = len(w.grid.recs) // 2
    huge = (w.huge_key_at.absolute("odd"), len(w.huge_key)) + HUGE_VALUE
    recs = np.concatenate([hc.shift_recs(w.grid.recs[:mid], w.grid_at.absolute("at_2g")), hc.fc.recs_of([huge]),
                           hc.shift_recs(w.grid.recs[mid:], w.grid_at.absolute("at_4g"))])
    assert huge[0] > B32 and HUGE_VALUE[1] > B32 and B31 < int(recs[:mid, 0].min()) < int(recs[:mid, 0].max()) < B32
    assert int(recs[mid + 1:, 0].min()) > B32
    assert big.h[huge[0]:huge[0] + huge[1]].tobytes() == w.huge_key
    exp = hc.packed_pieces(big.h, recs, UUID, 2, 9)
    n, size = len(recs), exp.file_bytes
    assert int((exp.recs[:, 0] > U64(B32)).sum()) == n - mid - 1       # half of the records lie above 2^32 in the file
    assert exp.pointers_at > B32 and [b[2] for b in exp.bodies] == [HUGE_VALUE[1]]
    with np.errstate(over="ignore"):
        assert repack.device_pack_bound(n, int(recs[:, 1].sum(dtype=U64)), int(recs[:, 3].sum(dtype=U64))) >= size
    whole, out = _fenced(size + 64, big.dev)
    assert out.data_ptr() % 16 == 0
    _, res = repack.device_pack(big.d, _dev_recs(recs, big.dev), UUID, 2, 9, out=out)
    assert _words(res.cpu().numpy()) == exp.res
    assert _canary_on_device(whole[PAD + size:]) and _canary_on_device(whole[:PAD])
    _packed_equal(big, out, exp, "pack")
    print(f"pack beyond 4 GiB: {time.perf_counter() - t0:.2f} s")


# ------------------------------------------------------------------ g. records
@pytest.mark.parametrize("block,tile", [(0, 0), (65536, 4096)], ids=["default", "b65536_t4096"])
def test_records_beyond_4gib(big, block, tile):
    t0 = time.perf_counter()
    off, size = big.images[0]
    h = big.lists[0]
    n = len(h)
    big_one = int(np.argmax(h[:, 3]))
    assert int(h[big_one, 3]) > B32 and big_one < n - 1 and int(h[big_one + 1:, 0].min()) > B32
    end, take = _trajectory(big.h[off:off + size], h, zsfile.END)
    cap = n + 8
    fr, recs = _fenced(32 * cap, big.dev)
    fs, res = _fenced(8 * zsfile.RECORDS_RES_WORDS, big.dev)
    zsfile.device_records(big.d[off:off + size], A, cap=cap, block_bytes=block, tile_bytes=tile,
                          out=(recs.view(torch.int64).view(cap, 4), res.view(torch.int64)))
    r = _inside(fs, 8 * zsfile.RECORDS_RES_WORDS).view(U64)
    got = _inside(fr, 32 * cap).view(U64).reshape(cap, 4)
    assert _words(r) == [zsfile.END, n, end] + _folds(h) + [take, 0, 0, 0], (r, end, take)
    assert np.array_equal(got[:n], h)
    assert bool((got[n:].view(np.uint8) == CANARY).all())
    print(f"records beyond 4 GiB ({block}, {tile}): {time.perf_counter() - t0:.2f} s")


# ------------------------------------------------------------------ h. records_multi and walk_multi
def test_records_multi_and_walk_multi_beyond_4gib(big):
    t0 = time.perf_counter()
    descs = big.images
    assert sum(off > B32 for off, _ in descs) == 2
    # the lister: the per-image host lists plus the image offsets, the rows and totals folded in numpy
    recs, rows, first = [], [], 0
    for (at, size), h in zip(descs, big.lists):
        end, take = _trajectory(big.h[at:at + size], h, zsfile.END)
        rows.append([zsfile.END, len(h), end] + _folds(h) + [take, first, 0, 0])
        recs.append(hc.shift_recs(h, at))
        first += len(h)
    recs = np.concatenate(recs)
    assert int(recs[:, 0].max()) > B32 + 5 * MIB
    _records_check(_records_run(big.d, descs, cap=first + 8), (recs, np.array(rows, U64), [first] + _folds(recs) + [0]))
    # the walk: the per-image host walks plus the image offsets
    offs, lens, imgs, rows, first = [], [], [], [], 0
    for j, ((at, size), (off, ln, rc, end)) in enumerate(zip(descs, big.walks)):
        assert rc == zsfile.END and end == size
        rows.append([rc, len(off), end, int(ln.max()), int(ln.min()),
                     _first_unaligned(big.h[at:at + size], rc, end, len(off)), first, 0])
        offs.append(off + U64(at))
        lens.append(ln)
        imgs.append(np.full(len(off), j, np.uint32))
        first += len(off)
    ln = np.concatenate(lens)
    assert int(ln.max()) > B32 and int(np.concatenate(offs).max()) > B32 + 5 * MIB
    _walk_check(_walk_run(big.d, descs, cap=first + 8),
                (np.concatenate(offs), ln, np.concatenate(imgs), np.array(rows, U64), [first, int(ln.max()), int(ln.min())]))
    print(f"records_multi and walk_multi beyond 4 GiB: {time.perf_counter() - t0:.2f} s")


# ------------------------------------------------------------------ i. end to end
@pytest.mark.parametrize("drop", [False, True], ids=["keep_deletes", "drop_deletes"])
def test_repack_beyond_4gib(big, drop):
    t0 = time.perf_counter()
    arena_lists = [(hc.shift_recs(h, at), 0) for (at, _), h in zip(big.images, big.lists)]
    merged, mres = hc.merge_model(big.h, arena_lists, drop)
    assert int(merged[:, 3].max()) == wi.HUGE_VALUE and int(merged[:, 0].max()) > B32 and mres[6] + mres[7] > 0
    exp = hc.packed_pieces(big.h, merged, UUID, 3, 5)
    assert exp.file_bytes > B32 and exp.pointers_at > B32 and int((exp.recs[:, 0] > U64(B32)).sum()) >= 1
    image, rep = repack.device_repack(big.d, big.images, [A, A, F], UUID, 3, 5, drop_deletes=drop)
    assert (rep["records_in"], rep["records_out"], rep["superseded"], rep["deletes_dropped"]) == \
        (mres[2], mres[1], mres[6], mres[7])
    assert rep["pack"] == exp.res and image.numel() == exp.file_bytes
    _packed_equal(big, image, exp, ("repack", drop))
    print(f"repack beyond 4 GiB (drop_deletes={drop}): {time.perf_counter() - t0:.2f} s")
