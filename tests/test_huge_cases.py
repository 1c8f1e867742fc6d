"""tests/huge_cases.py checked on the CPU: the piece builder's packed file
against tests/pack_cases.packed_file byte for byte, and the host twins
(zscrc_zs_find, zscrc_zs_scan, zscrc_zs_gather) over a lazily mapped arena of
2^32 + 768 MiB + 77 bytes, lists and queries beyond 2^31 and 2^32, against the
Python models' results moved there."""
import time

import numpy as np
import pytest

from oracle import oracle
from tests import find_cases as fc
from tests import gather_cases as gc
from tests import huge_cases as hc
from tests import pack_cases as pc
from tests import records_images as ri
from zeroskip_amd import repack, zsfile

U64 = np.uint64


def _words(a) -> list:
    return [int(v) for v in np.asarray(a).view(U64).ravel()]


# ------------------------------------------------------------------ the piece builder
def _pieces_equal(src: bytes, recs, want: bytes, uuid, startidx, endidx):
    host = np.frombuffer(src or b"\0", np.uint8)
    p = hc.packed_pieces(host, recs, uuid, startidx, endidx)
    assert p.file_bytes == len(want)
    assert p.assembled(host) == want
    cols, rc = repack.records(want, zsfile.PACKED)
    r = fc.recs_of(recs)
    if bool(((r[:, 2] == U64(hc.U64_MAX)) & (r[:, 1] > U64(65535))).any()):
        assert rc == zsfile.TRUNCATED       # a long delete record: the reference's form of it cannot be listed
    else:
        assert rc == 0 and np.array_equal(p.recs, np.ascontiguousarray(cols.T).reshape(-1, 4))
    off, ln, prc = zsfile.packed_spans(want)
    assert prc == 0 and p.res[:4] == [0, len(p.recs), len(want), int(ln[0])] and p.pointers_at == int(off[1])
    assert p.res[4] == oracle.crc32c_hw(0, want[int(off[0]):int(off[0] + ln[0])])
    assert p.res[5] == oracle.crc32c_hw(0, want[int(off[1]):int(off[1] + ln[1])])
    assert p.res[7] == int.from_bytes(want[-4:], "big")
    assert p.res[6] == int.from_bytes(want[int(off[1]) - 4:int(off[1])], "big")
    return p


def test_piece_builder_equals_the_packed_file():
    bodies = 0
    for c in pc.small_cases():
        p = _pieces_equal(c.src, c.recs, c.want, c.uuid, c.startidx, c.endidx)
        bodies += len(p.bodies)
    assert bodies > 0                                   # values that stayed in the source among them (70 KB, 1,000 B)
    img, pairs = ri.packed_400()
    recs, rc = ri.host_records(img, zsfile.PACKED)
    assert rc == 0 and int(recs[:, 3].max()) == (16 << 20) + 9
    p = _pieces_equal(img, recs, img, img[12:28], 1, 9)
    # the long value went through the threaded parts and the oracle's combine; its record has the long header
    assert [n for _, _, n in p.bodies] == [(16 << 20) + 9] and len(hc._big_crcs) >= 1


def test_long_span_crc_in_parts():
    """hc.span_crc's parts and folds against one call of the oracle over the same bytes."""
    a = np.random.default_rng(8).integers(0, 256, (130 << 20) + 5, dtype=np.uint8)
    assert hc.span_crc(a, 3, a.size - 3) == oracle.crc32c_hw(0, a[3:])
    assert hc.span_crc(a, 1, 64 << 20) == oracle.crc32c_hw(0, a[1:1 + (64 << 20)])


# ------------------------------------------------------------------ the host twins
@pytest.fixture(scope="module")
def arena():
    w = hc.world()
    w.layout.check()
    a = np.zeros(hc.ARENA_BYTES, np.uint8)

    def put(off, b):
        a[off:off + len(b)] = b
    w.layout.fill(put)
    return w, a


def test_layout_puts_a_key_byte_on_each_boundary(arena):
    w, a = arena
    for c, p in w.merge:
        for place, bound in (("at_2g", hc.B31), ("at_4g", hc.B32)):
            assert p.P[place] + p.key == bound and p.P[place] < bound < p.P[place] + p.size
        assert p.P["odd"] % 2 == 1 and p.P["odd"] > hc.B32 + (1 << 29)
        v = p.view(a)
        for place in hc.PLACES:
            assert v[p.P[place]:p.P[place] + p.size].tobytes() == c.src, (c.name, place)
    long_keys = [p for c, p in w.merge if c.name == "long_keys"][0]
    assert long_keys.key >= 35_000 and long_keys.size > 140_000


@pytest.mark.parametrize("carry", hc.CARRIES)
def test_host_find_beyond_4gib(arena, carry):
    w, a = arena
    t0 = time.perf_counter()
    seen_lo = seen_hi = False
    for c, p, qp in w.find:
        want, wres = c.model()
        src, qsrc = p.view(a), qp.view(a)
        for place in hc.PLACES:
            P, Q = p.P[place], qp.P[place]
            levels = hc.carried(c.levels, P, carry)
            queries = hc.shift_queries(c.queries, Q)
            hc.expect_crossing(levels, place, c.name)
            hc.expect_crossing([(queries, 0)], place, c.name)
            seen_lo |= place == "at_2g"
            seen_hi |= int(max(int(r[:, 0].max()) + b for r, b in levels if len(r))) > 1 << 32 and \
                int(queries[:, 0].max()) > 1 << 32
            hits, res = zsfile.find(src, levels, qsrc, queries)
            what = (c.name, place, carry)
            assert _words(res) == wres, (what, res)
            assert hits.view(U64).tobytes() == hc.shift_hits(want, P).tobytes(), what
    assert seen_lo and seen_hi
    print(f"host find beyond 4 GiB ({carry}): {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("carry", hc.CARRIES)
def test_host_scan_beyond_4gib(arena, carry):
    w, a = arena
    t0 = time.perf_counter()
    for c, p, qp in w.scan:
        src, qsrc = p.view(a), qp.view(a)
        for keep in (False, True):
            wrows, woffs, wseqs, wres = c.model(keep)
            for place in hc.PLACES:
                P, Q = p.P[place], qp.P[place]
                levels = hc.carried(c.levels, P, carry)
                queries = hc.shift_queries(c.queries, Q)
                hc.expect_crossing(levels, place, c.name)
                hc.expect_crossing([(queries, 0)], place, c.name)
                if place == "odd":
                    assert int(max(int(r[:, 0].max()) + b for r, b in levels if len(r))) > 1 << 32
                    assert int(queries[:, 0].max()) > 1 << 32
                rows, offs, seqs, res = zsfile.scan(src, levels, qsrc, queries, keep_deletes=keep)
                what = (c.name, place, carry, keep)
                assert _words(res) == wres, (what, res)
                assert rows.view(U64).tobytes() == hc.shift_recs(wrows, P).tobytes(), what
                assert offs.view(U64).tobytes() == woffs.tobytes() and seqs.view(U64).tobytes() == wseqs.tobytes(), what
    print(f"host scan beyond 4 GiB ({carry}): {time.perf_counter() - t0:.2f} s")


def test_host_gather_beyond_4gib(arena):
    """The gather's items carry their offsets themselves (there is no base):
    the small cases record-carried, and the find cases' hits, which a
    base-carried lookup has rebased, gathered from the lists' own view."""
    w, a = arena
    t0 = time.perf_counter()
    for c, p in w.gather:
        values, offs, crcs, res = c.model()
        o = offs.tolist()
        assert crcs.tolist() == [oracle.crc32c_hw(0, values[o[i]:o[i + 1]]) if o[i + 1] > o[i] else 0
                                 for i in range(c.nq)]
        for place in hc.PLACES:
            items = hc.shift_items(c.items, p.P[place])
            val = items[gc.kinds(items)[0]]
            assert int((val[:, 2] + val[:, 3]).max()) > (1 << 31 if place == "at_2g" else 1 << 32), (c.name, place)
            assert place != "odd" or int(val[:, 2].min()) > 1 << 32
            hv, ho, hcrc, hr = zsfile.gather(p.view(a), items, crcs=True)
            what = (c.name, place)
            assert _words(hr) == res, (what, hr)
            assert hv.tobytes() == values.tobytes() and ho.view(U64).tobytes() == offs.tobytes(), what
            assert hcrc.tobytes() == crcs.tobytes(), what
    for c, p, qp in w.find:
        want, _ = c.model()
        values, offs, crcs, res = gc.model(c.src, want)
        for place in ("at_4g", "odd"):
            items = hc.shift_hits(want, p.P[place])
            hv, ho, hcrc, hr = zsfile.gather(p.view(a), items, crcs=True)
            assert _words(hr) == res and hv.tobytes() == values.tobytes() and hcrc.tobytes() == crcs.tobytes(), c.name
            assert ho.view(U64).tobytes() == offs.tobytes(), c.name
    print(f"host gather beyond 4 GiB: {time.perf_counter() - t0:.2f} s")
