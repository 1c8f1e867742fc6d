"""The device lookup (zscrc_device_find, zeroskip_amd/csrc/zscrc_find.hip)
against the model of tests/find_cases.py (bisect_left over the levels' key
bytes) and against the host search, at every table size.  Hits sit in a
canary-filled buffer between fences: the fences, and on a refused call every
hit byte, must still hold the canary."""
import os

import numpy as np
import pytest
import torch

from oracle import zs_format as zf
from tests import devmem as dm
from tests import find_cases as fc
from tests.devmem import CANARY
from tests.images import REF, U64_MAX, UUIDSTR
from zeroskip_amd import zsfile

pytestmark = pytest.mark.gpu

SPLITS = [1, 2, 64, 2048, 0]      # no table, the smallest, a middle one, the largest, the default


def _find(case, dev, splitters=0, check_order=False, scratch=None, dev_in=None, shift=0, qshift=0):
    """device_find into canary rows between fences: (hits uint64 [nq, 4], res uint64 [8])."""
    d_src, levels, d_qsrc, queries = dev_in or dm.dev_in(case, dev, shift, qshift)
    nq = int(queries.shape[0])
    whole, out = dm.fenced(32 * nq, dev)
    res = torch.full((8,), -6, dtype=torch.int64, device=dev)
    zsfile.device_find(d_src, levels, d_qsrc, queries, check_order=check_order, splitters=splitters,
                       out=(out.view(torch.int64).view(nq, 4), res), scratch=scratch)
    return dm.inside(whole, 32 * nq, case.name).view(np.uint64).reshape(nq, 4), res.cpu().numpy().view(np.uint64)


def _same(case, dev, splits=SPLITS, check_order=False, shift=0, qshift=0, want=None):
    """The case at every table size: equal byte for byte, and equal to the model."""
    want, wres = want or case.model()
    dev_in = dm.dev_in(case, dev, shift, qshift)
    for s in splits:
        got, r = _find(case, dev, s, check_order, dev_in=dev_in)
        what = (case.name, s, check_order, shift, qshift)
        assert [int(v) for v in r] == wres, (what, r, wres)
        assert got.tobytes() == want.tobytes(), (what, np.argwhere(got != want)[:4].tolist())
    return wres


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in fc.small_cases()}


# ------------------------------------------------------------------ record counts
def test_record_counts_around_the_table_sizes(gpu, cases):
    """0 .. 3 records, and S - 1, S, S + 1, 2 S + 1, 3 (S + 1) - 1 for S = 2 and 64."""
    for n in (0, 1, 2, 3, 5, 8, 63, 64, 65, 129, 194):
        c = cases["n%d" % n]
        assert c.n == n
        r = _same(c, gpu)
        assert r[2] + r[3] == n and sum(r[2:6]) == r[1] > 2 * n


def test_record_counts_around_the_largest_table(gpu):
    for n in (2047, 2048, 2049, 4097):
        _same(fc.counted_case(n), gpu)


# ------------------------------------------------------------------- query counts
def test_query_counts(gpu, cases):
    c = cases["n194"]
    for nq in (0, 1, 63, 64, 65, 257):
        sub = fc.FindCase("nq%d" % nq, c.src, c.levels, c.qsrc, c.queries[:nq])
        assert len(sub.queries) == nq
        _same(sub, gpu)
    hits, res = zsfile.device_find(*dm.dev_in(fc.FindCase("nq0", c.src, c.levels, c.qsrc, c.queries[:0]), gpu))
    assert tuple(hits.shape) == (0, 4) and [int(v) for v in res.cpu()] == [0] * 8


def test_more_queries_than_the_grid_has_threads(gpu):
    """300,000 queries against a 1,280-record level: the grid-stride loop takes a second trip."""
    nq = 300_000
    assert nq > zsfile.FIND_GRID_THREADS == 1024 * 256
    src, recs = fc.counted_level(1280)
    keys = fc.level_keys(src, recs, 0)
    tail_blob, tail_q = fc.lay_queries(fc.probe_keys(keys[::5]))
    tail_q[:, 0] += np.uint64(len(src))
    idx = np.random.default_rng(3).integers(0, 1280, nq - len(tail_q))
    queries = np.concatenate([recs[idx], tail_q])              # the level's own records are queries as they stand
    assert len(queries) == nq
    blob = src + tail_blob
    want = np.zeros((nq, 4), np.uint64)
    want[:len(idx), 1] = idx
    want[:len(idx), 2:] = recs[idx, 2:]
    twant, tres = fc.model(src, [(recs, 0)], blob, tail_q)
    want[len(idx):] = twant
    dele = int((recs[idx, 2] == U64_MAX).sum())
    live = recs[idx][recs[idx, 2] != U64_MAX]
    wres = [0, nq, len(idx) - dele + tres[2], dele + tres[3], tres[4], 0, int(live[:, 3].sum()) + tres[6], 0]
    assert tres[4] > 100 and np.any(want[262_144:, 0] == fc.NONE)
    _same(fc.FindCase("second_trip", src, [(recs, 0)], blob, queries), gpu, splits=(1, 64, 0), want=(want, wres))


# --------------------------------------------------------------------------- keys
def test_shared_prefix_key_lengths_and_long_keys(gpu, cases):
    for name in ("shared_prefix", "key_lengths", "ends_at_last_byte", "long_keys"):
        _same(cases[name], gpu, check_order=True)


def test_every_key_offset_and_source_address(gpu, cases):
    """residue0..7 with the source at shifts 0..7, their query blobs at residues 0..7 and shifted too."""
    for r in range(8):
        for shift in range(8):
            _same(cases["residue%d" % r], gpu, splits=(64, 1), shift=shift, qshift=(shift * 3 + r) % 8)
    for shift in range(1, 8):
        _same(cases["ends_at_last_byte"], gpu, splits=(2, 1), shift=shift, qshift=8 - shift)
        _same(cases["long_keys"], gpu, splits=(2, 1), shift=shift, qshift=shift)


# ------------------------------------------------------------------------- levels
def test_no_levels_and_empty_levels(gpu, cases):
    for name in ("no_levels", "empty_levels"):
        r = _same(cases[name], gpu)
        assert r[4] == r[1] == len(cases[name].queries)          # nothing is found, every lower bound 0
        assert cases[name].model()[0][:, 1:].tolist() == [[0, 0, 0]] * r[1]


def test_deletes_values_and_the_last_level(gpu, cases):
    c = cases["deletes"]
    assert [len(r) for r, _ in c.levels] == [3, 0, 4]
    _same(c, gpu, check_order=True)
    got, res = _find(c, gpu, 2)
    a, b, cc, d = (got[i].tolist() for i in range(4))
    assert a[0] == 0 and a[2] == U64_MAX                     # a delete in level 0 over a value in level 2
    assert b[0] == 0 and c.src[b[2]:b[2] + b[3]] == b"new"   # a value in level 0 over a delete in level 2
    assert cc[0] == 2 and c.src[cc[2]:cc[2] + cc[3]] == b"last"   # only the last level holds it
    assert d == [fc.NONE, 3, 0, 0]                           # no level does: the last level's lower bound
    assert [int(v) for v in res] == [0, 8, 4, 1, 3, 0, 9, 0]
    # the last level empty: the lower bound of a key that is not found is 0
    tail = fc.FindCase("empty_last", c.src, c.levels + [(fc.recs_of([]), 0)], c.qsrc, c.queries)
    assert tail.model()[0][3].tolist() == [fc.NONE, 0, 0, 0]
    _same(tail, gpu)


def test_one_list_twice_with_two_bases(gpu, cases):
    c = cases["twice"]
    want, wres = c.model()
    found = want[want[:, 0] != fc.NONE]
    assert len(found) >= len(c.levels[0][0]) and bool((found[:, 0] == 0).all())     # level 0 wins every key
    assert int(found[:, 2].max()) < len(c.src) // 2
    _same(c, gpu)
    # the other way round the hits point into the arena's second half
    other = fc.FindCase("twice_reversed", c.src, c.levels[::-1], c.qsrc, c.queries)
    assert int(other.model()[0][0, 2]) >= len(c.src) // 2
    _same(other, gpu)


# -------------------------------------------------------------------- bad records
def test_records_outside_the_source(gpu, cases):
    """The offending record lies in levels that no query's search reaches: level 0 holds every query."""
    c = cases["n194"]
    size, recs = len(c.src), c.levels[0][0]
    q = recs[[3, 60, 120]]
    d_q, d_src = dm.dev_recs(q, gpu), dm.dev_bytes(c.src, gpu)

    def bad(changes, first, base=0):
        r = recs.copy()
        for i, col, v in changes:
            r[i, col] = v
        case = fc.FindCase("bad", c.src, [(q, 0), (r[:100], base), (r[100:], base)], c.src, q)
        dev_in = (d_src, [(dm.dev_recs(x, gpu), b) for x, b in case.levels], d_src, d_q)
        for s in (1, 64):
            got, res = _find(case, gpu, s, dev_in=dev_in)
            assert [int(v) for v in res] == [fc.EINVAL64, 3 + first, 0, 0, 0, 0, 0, 0], (changes, s, res)
            assert bool((got.view(np.uint8) == CANARY).all()), changes

    bad([(9, 0, size - 11)], 9)                                      # a 12-byte key that ends one byte past the source
    bad([(150, 2, size - 1), (150, 3, 2)], 150)                      # a value off the end
    bad([(193, 0, U64_MAX - 3)], 193)                                # an offset near 2^64
    bad([(0, 1, U64_MAX)], 0)                                        # key_len = 2^64 - 1
    bad([(150, 2, U64_MAX - 1)], 150)                                # a value offset that is almost DELETED
    bad([(190, 1, U64_MAX), (150, 0, size + 1), (101, 3, size + 1), (160, 0, U64_MAX - 3)], 101)
    bad([], 0, base=size)                                            # a base that moves every key off the end
    bad([], 0, base=U64_MAX - 5)                                     # a base whose sum with an offset wraps


# -------------------------------------------------------------------- bad queries
def test_bad_queries_among_good_ones(gpu, cases):
    c = cases["n65"]
    q = c.queries.copy()
    size = len(c.qsrc)
    q[3, 1] = size - int(q[3, 0]) + 1       # ends one byte past the query bytes
    q[10, 0] = U64_MAX - 3                  # an offset near 2^64
    q[20, 1] = U64_MAX                      # key_len = 2^64 - 1
    bad = fc.FindCase("badq", c.src, c.levels, c.qsrc, q)
    want, wres = bad.model()
    assert wres[5] == 3 and np.flatnonzero(want[:, 0] == fc.BAD_QUERY).tolist() == [3, 10, 20]
    assert want[[3, 10, 20], 1:].tolist() == [[0, 0, 0]] * 3
    _same(bad, gpu)


# -------------------------------------------------------------------- CHECK_ORDER
def test_check_order(gpu, cases):
    c = cases["n65"]
    recs = c.levels[0][0]
    swapped = recs.copy()
    swapped[[30, 31]] = swapped[[31, 30]]
    equal = recs.copy()
    equal[41] = equal[40]
    for r, first in ((swapped, 31), (equal, 41)):
        case = fc.FindCase("unsorted", c.src, [(recs[:7], 0), (r, 0)], c.qsrc, c.queries)   # seq counts level 0's 7
        dev_in = dm.dev_in(case, gpu)
        for s in (1, 2, 64):
            got, res = _find(case, gpu, s, check_order=True, dev_in=dev_in)
            assert [int(v) for v in res] == [fc.EINVAL64, 7 + first, 0, 0, 0, 0, 0, 1], (s, res)
            assert bool((got.view(np.uint8) == CANARY).all())
            # without the flag the list is searched all the same, inside its bounds; the hits are unspecified
            need = zsfile.device_find_scratch_bytes(2, s)
            whole, scratch = dm.fenced(need, gpu)
            got, res = _find(case, gpu, s, scratch=scratch, dev_in=dev_in)
            assert int(res[0]) == 0 and int(res[1]) == len(c.queries) and sum(int(v) for v in res[2:6]) == int(res[1])
            assert dm.intact(whole, need)
    # a bounds offence takes precedence over an earlier order offence
    r = swapped.copy()
    r[50, 1] = U64_MAX
    _, res = _find(fc.FindCase("both", c.src, [(r, 0)], c.qsrc, c.queries), gpu, 64, check_order=True)
    assert [int(v) for v in res] == [fc.EINVAL64, 50, 0, 0, 0, 0, 0, 0]
    # a descending step across a level boundary is no offence
    _same(fc.FindCase("boundary", c.src, [(recs[30:], 0), (recs[:30], 0)], c.qsrc, c.queries), gpu, check_order=True)


# --------------------------------------------- scratch, streams and determinism
def test_caller_scratch_fenced(gpu, cases):
    for name, s in (("n194", 64), ("deletes", 2048), ("no_levels", 0), ("twice", 1), ("n65", 2)):
        c = cases[name]
        need = zsfile.device_find_scratch_bytes(len(c.levels), s)
        assert need > 0
        whole, scratch = dm.fenced(need, gpu)
        assert scratch.data_ptr() % 16 == 0
        want, wres = c.model()
        got, r = _find(c, gpu, s, scratch=scratch)
        assert [int(v) for v in r] == wres and got.tobytes() == want.tobytes(), name
        assert dm.intact(whole, need), name


def test_library_scratch_behind_a_walk_on_another_stream(gpu, cases):
    """A walk and a lookup on two streams share the library's scratch, ordered by its event."""
    from tests import records_images as ri
    d_img = dm.dev_bytes(ri.wellformed(), gpu)

    def listed(walked):
        off, ln, res = (t.cpu().numpy() for t in walked)
        return off[:int(res[1])].tolist(), ln[:int(res[1])].tolist(), res.tolist()

    want_walk = listed(zsfile.device_walk(d_img))
    assert want_walk[2][1] > 0
    c = cases["n194"]
    dev_in = dm.dev_in(c, gpu)
    s1, s2 = torch.cuda.Stream(device=gpu), torch.cuda.Stream(device=gpu)
    torch.cuda.synchronize(gpu)
    want, wres = c.model()
    for _ in range(3):
        with torch.cuda.stream(s1):
            walked = zsfile.device_walk(d_img)
        with torch.cuda.stream(s2):
            hits, res = zsfile.device_find(*dev_in, splitters=64)
        torch.cuda.synchronize(gpu)
        assert [int(v) for v in res.cpu().numpy().view(np.uint64)] == wres
        assert hits.cpu().numpy().view(np.uint64).tobytes() == want.tobytes()
        assert listed(walked) == want_walk


def test_two_runs_bit_for_bit(gpu, cases):
    for name, s in (("n194", 64), ("key_lengths", 0), ("deletes", 2)):
        c = cases[name]
        dev_in = dm.dev_in(c, gpu)
        a = _find(c, gpu, s, dev_in=dev_in)
        b = _find(c, gpu, s, dev_in=dev_in)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# -------------------------------------------------------------- reference fixture
def test_reference_packed_file(gpu):
    img = open(os.path.join(REF, "packed.zs"), "rb").read()
    d_img = dm.dev_bytes(img, gpu)
    recs, rres = zsfile.device_records(d_img, zsfile.PACKED)
    n = int(rres[1])
    level = recs[:n].contiguous()
    keys = [k for k, _ in zf.packed_records(img)]
    assert n == len(keys) > 100
    host_level = level.cpu().numpy().view(np.uint64)
    near = [k + b"\x00" for k in keys] + [k[:-1] for k in keys if k]
    qsrc, queries = fc.lay_queries(near, residue=5)
    d_qsrc, d_q = dm.dev_bytes(qsrc, gpu), dm.dev_recs(queries, gpu)
    for s in SPLITS:
        # every key at its own index: the level is its own query list
        hits, res = zsfile.device_find(d_img, [(level, 0)], d_img, level, splitters=s, check_order=True)
        whits, wres = zsfile.find(img, [(host_level, 0)], img, host_level, check_order=True)
        assert hits.cpu().numpy().tobytes() == whits.tobytes() and res.cpu().numpy().tolist() == wres.tolist()
        assert whits[:, 0].tolist() == [0] * n and whits[:, 1].tolist() == list(range(n))
        # the host test's queries: equal to the host result
        hits, res = zsfile.device_find(d_img, [(level, 0)], d_qsrc, d_q, splitters=s)
        whits, wres = zsfile.find(img, [(host_level, 0)], qsrc, queries)
        assert hits.cpu().numpy().tobytes() == whits.tobytes() and res.cpu().numpy().tolist() == wres.tolist()
        assert int(wres[4]) > n


def test_reference_repack_inputs_as_levels(gpu):
    """repack2's two packed files as levels, the newer first: every key of either file."""
    d = os.path.join(REF, "repack2")
    newer = open(os.path.join(d, "zeroskip-%s-8-9" % UUIDSTR), "rb").read()
    older = open(os.path.join(d, "zeroskip-%s-4-7" % UUIDSTR), "rb").read()
    arena = newer + bytes(-len(newer) % 64) + older
    at = [0, len(arena) - len(older)]
    d_arena = dm.dev_bytes(arena, gpu)
    levels = []
    for off, img in zip(at, (newer, older)):
        recs, res = zsfile.device_records(d_arena[off:off + len(img)], zsfile.PACKED)
        levels.append((recs[:int(res[1])].contiguous(), off))
    host_levels = [(r.cpu().numpy().view(np.uint64), b) for r, b in levels]
    keys = sorted(set(k for img in (newer, older) for k, _ in zf.packed_records(img)))
    assert len(keys) < sum(len(r) for r, _ in host_levels)           # some keys are in both files
    qsrc, queries = fc.lay_queries(keys)
    want, wres = fc.model(arena, host_levels, qsrc, queries)
    assert wres[4] == 0 and set(want[:, 0].tolist()) == {0, 1}
    values = dict(zf.packed_records(older))
    values.update(dict(zf.packed_records(newer)))
    for k, (_, _, vo, vl) in zip(keys, want.tolist()):
        assert (None if vo == U64_MAX else arena[vo:vo + vl]) == values[k]
    d_qsrc, d_q = dm.dev_bytes(qsrc, gpu), dm.dev_recs(queries, gpu)
    for s in SPLITS:
        hits, res = zsfile.device_find(d_arena, levels, d_qsrc, d_q, splitters=s, check_order=True)
        assert hits.cpu().numpy().view(np.uint64).tobytes() == want.tobytes()
        assert [int(v) for v in res.cpu().numpy().view(np.uint64)] == wres


# -------------------------------------------------------------------------- scale
def test_a_million_records_and_a_million_queries(gpu):
    """2^20 + 1 records of the 8-byte big-endian keys 2 i, 2^20 random 8-byte keys in random order."""
    n, nq = (1 << 20) + 1, 1 << 20
    src = (2 * np.arange(n, dtype=np.uint64)).astype(">u8").view(np.uint8)
    recs = np.zeros((n, 4), np.uint64)
    recs[:, 0] = 8 * np.arange(n, dtype=np.uint64)
    recs[:, 1] = 8
    recs[:, 2] = recs[:, 0] + 8
    rng = np.random.default_rng(17)
    qv = rng.integers(0, 2 * n + 4, nq).astype(np.uint64)
    queries = np.zeros((nq, 4), np.uint64)
    queries[:, 0] = 8 * np.arange(nq, dtype=np.uint64)
    queries[:, 1] = 8
    at = np.searchsorted(2 * np.arange(n, dtype=np.uint64), qv, side="left")
    found = (at < n) & (qv % 2 == 0)
    want = np.zeros((nq, 4), np.uint64)
    want[:, 0] = np.where(found, 0, fc.NONE)
    want[:, 1] = at
    want[found, 2] = recs[at[found], 2]
    nf = int(found.sum())
    assert 0.4 * nq < nf < 0.6 * nq and int(at.max()) == n
    d_src, d_recs = torch.from_numpy(src).to(gpu), dm.dev_recs(recs, gpu)
    d_qsrc, d_q = torch.from_numpy(qv.astype(">u8").view(np.uint8)).to(gpu), dm.dev_recs(queries, gpu)
    for s in (0, 1, 2048):
        hits, res = zsfile.device_find(d_src, [(d_recs, 0)], d_qsrc, d_q, splitters=s, check_order=True)
        assert [int(v) for v in res.cpu()] == [0, nq, nf, 0, nq - nf, 0, 0, 0]
        assert np.array_equal(hits.cpu().numpy().view(np.uint64), want)


# ------------------------------------------------------------------------- random
@pytest.mark.parametrize("seed", range(20))
def test_random(gpu, seed):
    c = fc.random_find_case(seed)
    assert 1 <= len(c.levels) <= 4 and len(c.queries) == 3000
    _same(c, gpu, splits=(SPLITS[seed % 5], SPLITS[(seed + 2) % 5]), check_order=bool(seed & 1), qshift=seed % 8)
