"""The value gather on the device (zscrc_device_gather,
zeroskip_amd/csrc/zscrc_gather.hip) against the model of tests/gather_cases.py
(slices of the source, the oracle's CRCs) and against the host twin, at three
tile sizes.  Values, offsets and CRCs each sit in a canary-filled buffer between
fences: the fences, every value byte at or past the total, and on a refused
call every byte the call may not write, must still hold the canary."""
import os

import numpy as np
import pytest
import torch

from oracle import oracle
from oracle import zs_format as zf
from tests import devmem as dm
from tests import find_cases as fc
from tests import gather_cases as gc
from tests.devmem import CANARY
from tests.images import REF
from zeroskip_amd import zsfile

pytestmark = pytest.mark.gpu

TILES = [64, 1024, 0]       # the smallest, a middle one, the default
SLACK = 48                  # room behind the total that must stay untouched


def _gather(d_src, d_items, cap, tile=0, crcs=True, scratch=None, out_null=False):
    """device_gather into canary buffers between fences: (out uint8 [cap], offs
    uint64 [nq + 1], crcs uint32 [nq], res [8]) as they are afterwards."""
    dev, nq = d_src.device, int(d_items.shape[0])
    w_out, out = dm.fenced(cap, dev)
    w_offs, offs = dm.fenced(8 * (nq + 1), dev)
    w_crc, crc = dm.fenced(4 * nq, dev)
    res = torch.full((8,), -6, dtype=torch.int64, device=dev)
    assert out.data_ptr() % 16 == 0
    zsfile.device_gather(d_src, d_items, cap=0 if out_null else cap, tile_bytes=tile, scratch=scratch,
                         out=(None if out_null else out, offs.view(torch.int64),
                              crc.view(torch.int32) if crcs else None, res))
    what = (nq, cap, tile)
    return (dm.inside(w_out, cap, what), dm.inside(w_offs, 8 * (nq + 1), what).view(np.uint64),
            dm.inside(w_crc, 4 * nq, what).view(np.uint32), [int(v) for v in res.cpu().numpy().view(np.uint64)])


def _same(case, dev, tiles=TILES, shift=0, host=True, want=None):
    """The case at every tile size: equal byte for byte to the model (and so to
    each other), and to the host twin; nothing written at or past the total."""
    values, offs, crcs, res = want or case.model()
    total = res[3]
    d_src, d_items = dm.dev_bytes(case.src, dev, shift), dm.dev_recs(case.items, dev)
    for t in tiles:
        out, o, c, r = _gather(d_src, d_items, total + SLACK, t)
        what = (case.name, t, shift)
        assert r == res, (what, r, res)
        assert o.tobytes() == offs.tobytes(), (what, np.flatnonzero(o != offs)[:4].tolist())
        assert out[:total].tobytes() == values.tobytes(), (what, np.flatnonzero(out[:total] != values)[:4].tolist())
        assert bool((out[total:] == CANARY).all()), what        # the bound of the writes is the total itself
        assert c.tobytes() == crcs.tobytes(), (what, np.flatnonzero(c != crcs)[:4].tolist())
    if host:
        hv, ho, hc, hr = zsfile.gather(case.src, case.items, crcs=True)
        assert hv.tobytes() == values.tobytes() and ho.view(np.uint64).tobytes() == offs.tobytes()
        assert hc.tobytes() == crcs.tobytes() and [int(v) for v in hr.view(np.uint64)] == res
    return res


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in gc.small_cases()}


# -------------------------------------------------------------------- item counts
def test_item_counts(gpu, cases):
    for n in gc.COUNTS:
        c = cases["n%d" % n]
        assert c.nq == n
        r = _same(c, gpu)
        assert r[2] + r[4] + r[5] + r[6] == r[1] == n
    values, offs, crc, res = zsfile.device_gather(dm.dev_bytes(b"abc", gpu), dm.dev_recs(gc.items_of([]), gpu), crcs=True)
    assert values.numel() == 0 and offs.cpu().tolist() == [0] and crc.numel() == 0 and res.cpu().tolist() == [0] * 8


def test_a_million_short_items(gpu):
    """2^20 + 1 items of 0 to 3 bytes: the one-workgroup scan runs over more than 1,024 block sums."""
    c = gc.million_case()
    assert c.nq == (1 << 20) + 1 > 1024 * 1024
    values, offs, _, res = c.model(crcs=False)
    hv, ho, hc, hr = zsfile.gather(c.src, c.items, crcs=True)          # the CRCs: the host twin's, a sample the oracle's
    assert hv.tobytes() == values.tobytes() and ho.view(np.uint64).tobytes() == offs.tobytes()
    o = offs.tolist()
    vb = values.tobytes()
    for i in list(range(0, c.nq, 997)) + [c.nq - 1]:
        assert int(hc[i]) == (oracle.crc32c_hw(0, vb[o[i]:o[i + 1]]) if o[i + 1] > o[i] else 0)
    _same(c, gpu, tiles=(64, 0), host=False, want=(values, offs, hc, res))


# ------------------------------------------------------------------ value lengths
@pytest.mark.parametrize("tile", [64, 1024, zsfile.GATHER_DEFAULT_TILE])
def test_lengths_at_every_source_offset_and_address(gpu, tile):
    """0 .. 33 and tile - 1, tile, tile + 1, 3 tile + 5 from source offsets at
    every residue mod 16, from a source tensor at every address mod 16."""
    assert gc.tile_lengths(tile)[:10] == [0, 1, 7, 8, 9, 15, 16, 17, 31, 33]
    for r in range(16):
        case = gc.residue_case(tile, r)
        want = case.model()
        _same(case, gpu, tiles=(tile, 0), host=False, want=want)
        _same(case, gpu, tiles=(tile,), shift=(r * 5 + 3) % 16, host=False, want=want)
    for shift in range(16):
        _same(gc.residue_case(tile, 5), gpu, tiles=(tile,), shift=shift, host=shift == 0)


def test_every_output_residue_and_both_ends_of_the_source(gpu, cases):
    front = cases["front"]
    starts = front.model(crcs=False)[1][1:48:3] % np.uint64(16)
    assert set(starts.tolist()) == set(range(16))        # the 33-byte values start at every output residue
    _same(front, gpu)
    ends = cases["ends"]
    assert ends.items[1, 2] == 0 and int(ends.items[2, 2] + ends.items[2, 3]) == len(ends.src)
    for shift in (0, 1, 8, 15):
        _same(ends, gpu, shift=shift)
    _same(cases["lengths64"], gpu)


# ------------------------------------------------------------ items without a value
def test_items_without_a_value(gpu, cases):
    for name, word in (("only_misses", 5), ("only_deletes", 4), ("only_badq", 6)):
        r = _same(cases[name], gpu)
        assert r == [0, 300, 0, 0] + [300 if w == word else 0 for w in (4, 5, 6)] + [0]   # a total of 0: nothing written
    r = _same(cases["badq_among_good"], gpu)
    assert r[6] == 4 and r[2] + r[6] == 200
    c = cases["misses_between"]
    assert c.nq == 30_003 and c.items[0, 0] == gc.NONE and c.items[-1, 0] == gc.NONE
    assert _same(c, gpu)[2:6] == [3, 88, 0, 30_000]


def test_more_one_byte_values_than_a_stage_holds(gpu):
    c = gc.one_byte_case()
    assert c.nq >= 2 * 65536 and zsfile.GATHER_DEFAULT_TILE > zsfile.GATHER_STAGE   # a tile of them outruns a stage
    values, offs, _, res = c.model(crcs=False)
    assert res[2:4] == [c.nq, c.nq] and res[7] == 1
    hc = zsfile.gather(c.src, c.items, crcs=True)[2]
    assert [int(v) for v in hc[:2000]] == [oracle.crc32c_hw(0, bytes([b])) for b in values[:2000].tolist()]
    _same(c, gpu, tiles=(64, 1024, 0, 65536), want=(values, offs, hc, res))


def test_a_long_value_spans_many_runs(gpu):
    c = gc.long_value_case()
    assert int(c.items[2, 3]) == 3 * (1 << 20) + 5 and c.items[1].tolist() == c.items[3].tolist()
    r = _same(c, gpu, tiles=(64, 1024, 0, 65536))
    assert r[7] == 3 * (1 << 20) + 5


def test_the_copy_that_searches_offs_in_global_memory(gpu, cases, monkeypatch):
    """ZSCRC_GATHER_SEARCH=1: the measured alternative to the staged chunks gives the same bytes."""
    monkeypatch.setenv("ZSCRC_GATHER_SEARCH", "1")
    for name in ("n4097", "front", "ends", "misses_between", "lengths64", "only_misses"):
        _same(cases[name], gpu, tiles=(0,), host=False)
    _same(gc.long_value_case(), gpu, tiles=(0,), host=False)
    _same(gc.random_case(7), gpu, tiles=(0,), shift=7, host=False)


# --------------------------------------------------------------------- bad values
def test_values_outside_the_source(gpu, cases):
    case = cases["n4097"]
    size = len(case.src)
    val = np.flatnonzero(gc.kinds(case.items)[0])
    d_src = dm.dev_bytes(case.src, gpu)

    def bad(changes, first):
        items = case.items.copy()
        for i, off, ln in changes:
            items[i, 2:] = (off, ln)
        assert gc.model(case.src, items)[3] == [gc.EINVAL64, first, 0, 0, 0, 0, 0, 0]
        d_items = dm.dev_recs(items, gpu)
        for t in (64, 0):
            out, offs, crc, res = _gather(d_src, d_items, 1 << 17, t)
            assert res == [gc.EINVAL64, first, 0, 0, 0, 0, 0, 0], (changes, t, res)
            assert bool((out == CANARY).all()) and bool((offs.view(np.uint8) == CANARY).all()), changes
            assert crc.tolist() == [0] * case.nq

    a, b, c = int(val[3]), int(val[len(val) // 2]), int(val[-1])
    assert a < 1024 and a // 1024 != b // 1024 != c // 1024
    bad([(a, size - 4, 5)], a)                       # val_off + val_len one past the source
    bad([(b, size, 1)], b)                           # val_off >= src_size
    bad([(b, size + 1, 0)], b)
    bad([(c, 0, 1 << 63)], c)                        # val_len = 2^63
    bad([(c, gc.U64_MAX - 1, 3)], c)                 # an add that would wrap
    bad([(c, 1, size), (b, 9, size)], b)             # two bad items in different blocks: the smaller index
    # the same words under a miss or a bad query are never looked at
    items = case.items.copy()
    items[a], items[b] = gc.WILD_MISS, gc.WILD_BADQ
    _same(gc.GatherCase("wild", case.src, items), gpu, tiles=(64, 0))


# ----------------------------------------------------------------------- overflow
def test_overflow_and_the_sizing_call(gpu, cases):
    for case in (cases["n257"], gc.random_case(1)):
        values, offs, crcs, res = case.model()
        total = res[3]
        d_src, d_items = dm.dev_bytes(case.src, gpu), dm.dev_recs(case.items, gpu)
        for cap in (total - 1, 16):
            for t in (64, 0):
                out, o, c, r = _gather(d_src, d_items, cap, t)
                assert r == [gc.OVERFLOW] + res[1:] == case.model(cap=cap)[3], (case.name, cap, t)
                assert o.tobytes() == offs.tobytes()               # complete and equal to the model's
                assert bool((out == CANARY).all())                 # no byte of the output
                assert c.tolist() == [0] * case.nq                 # every CRC 0
        out, o, c, r = _gather(d_src, d_items, 0, out_null=True)  # the sizing call leaves the CRCs alone
        assert r == [gc.OVERFLOW] + res[1:] and o.tobytes() == offs.tobytes()
        assert bool((c.view(np.uint8) == CANARY).all())
        # cap=None: the wrapper's sizing call, the one word read, the allocation
        v, o, c, r = zsfile.device_gather(d_src, d_items, crcs=True)
        assert v.numel() == total and v.cpu().numpy().tobytes() == values.tobytes()
        assert c.cpu().numpy().view(np.uint32).tobytes() == crcs.tobytes() and int(r[0]) == 0


# --------------------------------------------------------------------------- CRCs
def test_without_crcs_the_same_values_and_offsets(gpu, cases):
    for name in ("n1025", "front", "misses_between"):
        case = cases[name]
        values, offs, _, res = case.model(crcs=False)
        d_src, d_items = dm.dev_bytes(case.src, gpu), dm.dev_recs(case.items, gpu)
        for t in TILES:
            out, o, c, r = _gather(d_src, d_items, res[3] + SLACK, t, crcs=False)
            assert r == res and o.tobytes() == offs.tobytes() and out[:res[3]].tobytes() == values.tobytes()
            assert bool((c.view(np.uint8) == CANARY).all())        # no CRC asked for, none written


# --------------------------------------------- scratch, streams and determinism
def test_caller_scratch_fenced(gpu, cases):
    for name, t in (("n4097", 64), ("n0", 0), ("misses_between", 1024), ("front", 0), ("only_misses", 0)):
        case = cases[name]
        need = zsfile.device_gather_scratch_bytes(case.nq, t)
        assert need > 0
        whole, scratch = dm.fenced(need, gpu)
        assert scratch.data_ptr() % 16 == 0
        values, offs, crcs, res = case.model()
        out, o, c, r = _gather(dm.dev_bytes(case.src, gpu), dm.dev_recs(case.items, gpu), res[3] + SLACK, t,
                               scratch=scratch)
        assert r == res and o.tobytes() == offs.tobytes() and out[:res[3]].tobytes() == values.tobytes(), name
        assert c.tobytes() == crcs.tobytes(), name
        dm.inside(whole, need, name)


def test_library_scratch_behind_a_walk_on_another_stream(gpu, cases):
    """A walk and a gather on two streams share the library's scratch, ordered by its event."""
    from tests import records_images as ri
    d_img = dm.dev_bytes(ri.wellformed(), gpu)

    def listed(walked):
        off, ln, res = (t.cpu().numpy() for t in walked)
        return off[:int(res[1])].tolist(), ln[:int(res[1])].tolist(), res.tolist()

    want_walk = listed(zsfile.device_walk(d_img))
    assert want_walk[2][1] > 0
    case = cases["n4097"]
    values, offs, crcs, res = case.model()
    d_src, d_items = dm.dev_bytes(case.src, gpu), dm.dev_recs(case.items, gpu)
    s1, s2 = torch.cuda.Stream(device=gpu), torch.cuda.Stream(device=gpu)
    torch.cuda.synchronize(gpu)
    for _ in range(3):
        with torch.cuda.stream(s1):
            walked = zsfile.device_walk(d_img)
        with torch.cuda.stream(s2):
            v, o, c, r = zsfile.device_gather(d_src, d_items, cap=res[3], crcs=True, tile_bytes=64)
        torch.cuda.synchronize(gpu)
        assert [int(x) for x in r.cpu().numpy().view(np.uint64)] == res
        assert v.cpu().numpy().tobytes() == values.tobytes() and o.cpu().numpy().view(np.uint64).tobytes() == offs.tobytes()
        assert c.cpu().numpy().view(np.uint32).tobytes() == crcs.tobytes()
        assert listed(walked) == want_walk


def test_two_runs_bit_for_bit(gpu, cases):
    for case, t in ((cases["n4097"], 64), (gc.random_case(3), 0), (cases["misses_between"], 1024)):
        d_src, d_items = dm.dev_bytes(case.src, gpu), dm.dev_recs(case.items, gpu)
        cap = case.model(crcs=False)[3][3] + SLACK
        a = _gather(d_src, d_items, cap, t)
        b = _gather(d_src, d_items, cap, t)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


# ------------------------------------------------------------- find, then gather
def test_device_get_on_the_find_cases(gpu):
    """A multi-get on every case of the lookup: the values the model's hits name,
    and the gather's counts against the find's."""
    n = 0
    for case in fc.small_cases():
        want_hits, wres = case.model()
        values, offs, crcs, _ = gc.model(case.src, want_hits)
        d_src = dm.dev_bytes(case.src, gpu)
        levels = [(dm.dev_recs(r, gpu), b) for r, b in case.levels]
        d_qsrc, d_q = dm.dev_bytes(case.qsrc, gpu), dm.dev_recs(case.queries, gpu)
        for cap in (None, len(values) + 16):
            v, o, c, hits, fres, gres = zsfile.device_get(d_src, levels, d_qsrc, d_q, cap=cap, crcs=True)
            f = [int(x) for x in fres.cpu().numpy().view(np.uint64)]
            g = [int(x) for x in gres.cpu().numpy().view(np.uint64)]
            assert f == wres and hits.cpu().numpy().view(np.uint64).tobytes() == want_hits.tobytes(), case.name
            assert g[0] == 0 and g[1] == len(case.queries)
            assert [g[2], g[3], g[4], g[5], g[6]] == [f[2], f[6], f[3], f[4], f[5]], case.name
            assert v.cpu().numpy()[:g[3]].tobytes() == values.tobytes(), case.name
            assert o.cpu().numpy().view(np.uint64).tobytes() == offs.tobytes(), case.name
            assert c.cpu().numpy().view(np.uint32).tobytes() == crcs.tobytes(), case.name
        n += g[2]
    assert n > 1000


# -------------------------------------------------------------- reference fixture
def test_reference_packed_file_as_a_record_list(gpu):
    img = open(os.path.join(REF, "packed.zs"), "rb").read()
    pairs = zf.packed_records(img)
    d_img = dm.dev_bytes(img, gpu)
    recs, rres = zsfile.device_records(d_img, zsfile.PACKED)
    n = int(rres[1])
    assert n == len(pairs) > 100
    level = recs[:n].contiguous()                              # a record list is a gather list as it stands
    host = level.cpu().numpy().view(np.uint64)
    case = gc.GatherCase("packed.zs", img, host)
    res = _same(case, gpu)
    values, offs, _, _ = case.model(crcs=False)
    o = offs.tolist()
    assert [values[o[i]:o[i + 1]].tobytes() for i in range(n)] == [val or b"" for _, val in pairs]
    assert res[2] == sum(val is not None for _, val in pairs) and res[5] == res[6] == 0


# ------------------------------------------------------------------------- random
@pytest.mark.parametrize("seed", range(20))
def test_random(gpu, seed):
    c = gc.random_case(seed)
    assert c.nq == 2000
    r = _same(c, gpu, shift=seed % 16)
    assert 0.2 * c.nq < c.nq - r[2] < 0.45 * c.nq and r[7] > 4000
