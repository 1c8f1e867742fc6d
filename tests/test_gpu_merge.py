"""The device merge (zscrc_device_merge, zeroskip_amd/csrc/zscrc_merge.hip)
against the few lines of Python of tests/merge_cases.py (sorted by (key bytes,
seq), the last of every run of equal keys), and device_repack's file against
the format oracle's and the host repack's, byte for byte.  Output lists are
canary-filled between fences: rows at and after min(n_out, cap) and the fences
must still hold the canary."""
import numpy as np
import pytest
import torch

from oracle import zs_format as zf
from tests import devmem as dm
from tests import merge_cases as mc
from tests.devmem import CANARY
from tests.images import EINVAL64, OVERFLOW, U64_MAX, UUID, UUIDSTR
from zeroskip_amd import repack, zsfile

pytestmark = pytest.mark.gpu

TILES = [64, 256, 0]
TILE_IDS = ["t64", "t256", "default"]


def _merge(case, dev, drop, cap, tile=0, shift=0, scratch=None, dev_in=None):
    """device_merge into `cap` canary rows between fences: (the rows uint64 [cap, 4], res uint64[8])."""
    d_src, lists = dev_in or (dm.dev_bytes(case.src, dev, shift), [(dm.dev_recs(r, dev), b) for r, b in case.lists])
    whole, out = dm.fenced(32 * cap, dev)
    _, res = repack.device_merge(d_src, lists, drop_deletes=drop, out=out.view(torch.int64).view(cap, 4),
                                 tile_records=tile, scratch=scratch)
    r = res.cpu().numpy().view(np.uint64)
    return dm.inside(whole, 32 * cap, case.name).view(np.uint64).reshape(cap, 4), r


def _same(case, dev, drop=False, tile=0, shift=0, slack=3, scratch=None, dev_in=None):
    """The case merged into n_out + slack rows equals the model; returns res."""
    want, wres = case.model(drop)
    got, r = _merge(case, dev, drop, len(want) + slack, tile, shift, scratch, dev_in)
    what = (case.name, drop, tile, shift)
    assert [int(v) for v in r] == wres, (what, r, wres)
    assert int(r[1]) + int(r[6]) + int(r[7]) == int(r[2]), what
    assert got[:len(want)].tolist() == want.tolist(), what
    assert bool((got[len(want):].view(np.uint8) == CANARY).all()), what      # nothing at or after n_out
    return r


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in mc.small_cases()}


# ------------------------------------------------------------- empty and single
def test_empty_and_one_record(gpu, cases):
    for name in ("no_lists", "empty_lists", "one_record"):
        for drop in (False, True):
            r = _same(cases[name], gpu, drop)
    assert [int(v) for v in _same(cases["no_lists"], gpu)] == [0] * 8
    # lists of no records between lists that hold some
    c = cases["deletes"]
    none = (np.zeros((0, 4), np.uint64), 77)
    mixed = mc.Case("mixed", c.src, [none, c.lists[0], none, none, c.lists[1], c.lists[2], none])
    assert mixed.model(False)[0].tolist() == c.model(False)[0].tolist()
    _same(mixed, gpu, tile=64)


def test_filled_lists_between_empty_ones_with_three_bases(gpu):
    """(empty, 3 records, empty, 1 record, empty): the index of a list among those that are not empty differs from
    the caller's at both ends and in the middle, and each staged descriptor must carry its own list's base."""
    img = mc.from_items("img", [(b"b", b"old"), (b"a", None), (b"c", b"3"), (b"b", b"new")])
    recs, size = img.lists[0][0], 128
    assert len(img.src) <= size
    copy = img.src + b"\xEE" * (size - len(img.src))
    none = np.zeros((0, 4), np.uint64)
    c = mc.Case("empty_3_empty_1_empty", b"\xEE" * size + copy + copy,
                [(none, 0), (recs[:3], size), (none, 2 * size), (recs[3:], 2 * size), (none, size)])
    assert len(c.src) == 384 and c.n == 4
    for drop in (False, True):
        r = _same(c, gpu, drop)
        _same(c, gpu, drop, tile=64)
        # a (a delete), b (the later list's, superseding one), c
        assert [int(r[i]) for i in (1, 2, 6, 7)] == ([2, 4, 1, 1] if drop else [3, 4, 1, 0])
    want = c.model(False)[0]
    assert c.pairs(want) == [(b"a", None), (b"b", b"new"), (b"c", b"3")]
    assert int(want[1, 0]) >= 2 * size > int(want[2, 0]) >= size


# ------------------------------------------------------------------ tile counts
@pytest.mark.parametrize("tile", TILES, ids=TILE_IDS)
def test_record_counts_around_the_tile(gpu, cases, tile):
    """tile - 1, tile, tile + 1, 2 tile + 1, 3 and 5 tiles of 64 and 256: a run without a partner."""
    for n in (63, 64, 65, 129, 192, 320, 255, 256, 257, 513, 768, 1280):
        _same(cases["n%d" % n], gpu, tile=tile)
    if tile == 0:
        for n in (2047, 2048, 2049, 4097, 6144, 10240):       # the same counts of the default tile (2048)
            _same(mc.counted(n), gpu)


# -------------------------------------------------------------------------- keys
@pytest.mark.parametrize("tile", TILES, ids=TILE_IDS)
def test_shared_prefix_and_key_lengths(gpu, cases, tile):
    for name in ("shared_prefix", "key_lengths", "ends_at_last_byte", "long_keys"):
        for drop in (False, True):
            _same(cases[name], gpu, drop, tile=tile)


def test_every_key_offset_and_source_address(gpu, cases):
    for r in range(8):
        for shift in range(8):
            _same(cases["residue%d" % r], gpu, tile=64, shift=shift)
    for shift in range(1, 8):
        _same(cases["ends_at_last_byte"], gpu, shift=shift)
        _same(cases["long_keys"], gpu, shift=shift)


def test_sorted_reversed_and_one_key(gpu, cases):
    for name in ("sorted", "reversed"):
        for tile in TILES:
            _same(cases[name], gpu, tile=tile)
    c = cases["one_key"]
    assert c.n == 500
    for drop in (False, True):
        r = _same(c, gpu, drop, tile=64)
        assert int(r[1]) == 1 and int(r[6]) == 499         # the winner is the last seq, across eight tiles
    assert c.model(False)[0][0].tolist() == c.rebased()[499].tolist()


def test_two_sorted_lists_of_1_and_1000(gpu, cases):
    for tile in TILES:
        for drop in (False, True):
            _same(cases["one_and_thousand"], gpu, drop, tile=tile)
    # the other way round the single record is the later one and wins
    c = cases["one_and_thousand"]
    _same(mc.Case("thousand_and_one", c.src, c.lists[::-1]), gpu, True, tile=64)


# ----------------------------------------------------------------------- deletes
def test_deletes_kept_and_dropped(gpu, cases):
    c = cases["deletes"]
    kept, dropped = _same(c, gpu, False, tile=64), _same(c, gpu, True, tile=64)
    # a, c, e end as deletes; b, d, f as values
    assert [int(kept[i]) for i in (1, 3, 6, 7)] == [6, 3, 5, 0]
    assert [int(dropped[i]) for i in (1, 3, 6, 7)] == [3, 0, 5, 3]
    assert [k for k, _ in c.pairs(c.model(True)[0])] == [b"b", b"d", b"f"]


def test_one_list_twice_with_two_bases(gpu, cases):
    c = cases["twice"]
    want, _ = c.model(False)
    assert int(want[:, 0].min()) >= len(c.src) // 2          # every winner is the second copy's
    for tile in (64, 0):
        _same(c, gpu, tile=tile)


# ------------------------------------------------------------------ bad records
def test_records_outside_the_source(gpu, cases):
    c = cases["n320"]
    size, recs = len(c.src), c.lists[0][0]

    def bad(changes, first, base=0):
        r = recs.copy()
        for i, col, v in changes:
            r[i, col] = v
        got, res = _merge(mc.Case("bad", c.src, [(r[:100], base), (r[100:], base)]), gpu, False, 330, tile=64)
        assert int(res[0]) == EINVAL64 and int(res[1]) == first and int(res[2]) == 320, (changes, res)
        assert [int(v) for v in res[3:]] == [0] * 5
        assert bool((got.view(np.uint8) == CANARY).all()), changes

    bad([(9, 0, size - 11)], 9)                                      # a 12-byte key that ends one byte past the source
    bad([(200, 2, size - 1), (200, 3, 2)], 200)                      # a value off the end
    bad([(319, 0, U64_MAX - 3)], 319)                                # an offset near 2^64
    bad([(0, 1, U64_MAX)], 0)                                        # key_len = 2^64 - 1
    bad([(150, 2, U64_MAX - 1)], 150)                                # a value offset that is almost DELETED
    bad([(310, 1, U64_MAX), (150, 0, size + 1), (101, 3, size + 1), (250, 0, U64_MAX - 3)], 101)
    bad([], 0, base=size)                                            # a base that moves every key off the end
    bad([], 0, base=U64_MAX - 5)                                     # a base whose sum with an offset wraps


# ---------------------------------------------------------------------- capacity
def test_capacity(gpu, cases):
    for name, drop in (("n320", False), ("deletes", True), ("one_record", False)):
        c = cases[name]
        want, wres = c.model(drop)
        n_out = len(want)
        _same(c, gpu, drop, tile=64, slack=0)                           # cap == n_out
        for cap in sorted({n_out - 1, n_out // 2, 0}):
            got, r = _merge(c, gpu, drop, cap, tile=64)
            assert [int(v) for v in r] == [OVERFLOW] + wres[1:], (name, cap, r)
            assert got.tolist() == want[:cap].tolist(), (name, cap)
        # the sizing call: no output at all, then the wrapper's own
        d_src, lists = dm.dev_bytes(c.src, gpu), [(dm.dev_recs(r, gpu), b) for r, b in c.lists]
        _, res = repack.device_merge(d_src, lists, drop_deletes=drop, out=torch.empty((0, 4), dtype=torch.int64,
                                                                                       device=gpu))
        assert [int(v) for v in res.cpu().numpy()] == [OVERFLOW] + wres[1:]
        out, res = repack.device_merge(d_src, lists, drop_deletes=drop)
        assert tuple(out.shape) == (n_out, 4) and out.cpu().numpy().view(np.uint64).tolist() == want.tolist()
        assert [int(v) for v in res.cpu().numpy()] == wres


# ------------------------------------------- scratch, streams and determinism
def test_caller_scratch_fenced(gpu, cases):
    for name, tile in (("n1280", 64), ("n513", 0), ("no_lists", 0), ("one_and_thousand", 256)):
        c = cases[name]
        need = repack.device_merge_scratch_bytes(c.n, tile)
        assert need > 0
        whole, scratch = dm.fenced(need, gpu)
        assert scratch.data_ptr() % 16 == 0
        _same(c, gpu, tile=tile, scratch=scratch)
        assert dm.intact(whole, need), name


def test_library_scratch_behind_a_walk_on_another_stream(gpu, cases):
    """A walk and a merge on two streams share the library's scratch, ordered by its event."""
    from tests import records_images as ri
    img = ri.wellformed()
    d_img = dm.dev_bytes(img, gpu)
    def walk():
        off, ln, res = zsfile.device_walk(d_img)
        return off, ln, res

    def listed(walked):
        off, ln, res = (t.cpu().numpy() for t in walked)
        return off[:int(res[1])].tolist(), ln[:int(res[1])].tolist(), res.tolist()

    want_walk = listed(walk())
    assert want_walk[2][1] > 0
    c = cases["n1280"]
    dev_in = (dm.dev_bytes(c.src, gpu), [(dm.dev_recs(r, gpu), b) for r, b in c.lists])
    s1, s2 = torch.cuda.Stream(device=gpu), torch.cuda.Stream(device=gpu)
    torch.cuda.synchronize(gpu)
    want, wres = c.model(False)
    for _ in range(3):
        with torch.cuda.stream(s1):
            walked = walk()
        with torch.cuda.stream(s2):
            out, res = repack.device_merge(*dev_in, out=torch.zeros((len(want), 4), dtype=torch.int64, device=gpu),
                                           tile_records=64)
        torch.cuda.synchronize(gpu)
        assert [int(v) for v in res.cpu().numpy()] == wres
        assert out.cpu().numpy().view(np.uint64).tolist() == want.tolist()
        assert listed(walked) == want_walk


def test_two_runs_bit_for_bit(gpu, cases):
    for name, tile in (("n1280", 64), ("key_lengths", 0)):
        c = cases[name]
        dev_in = (dm.dev_bytes(c.src, gpu), [(dm.dev_recs(r, gpu), b) for r, b in c.lists])
        a = _merge(c, gpu, False, c.n, tile, dev_in=dev_in)
        b = _merge(c, gpu, False, c.n, tile, dev_in=dev_in)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ------------------------------------------------- more blocks than one scan chunk
def test_more_blocks_than_one_scan_chunk(gpu):
    """1024 * 1024 + 1 records are 1,025 blocks of 1,024 entries: merge_scan_kernel takes a second chunk of
    block counts and merge_scatter_kernel's last block starts at a carried offset.  Record i is the 8-byte
    big-endian key i // 2 with an empty value: every key twice (the later record wins), the last one once."""
    n = 1024 * 1024 + 1
    n_out = n // 2 + 1
    src = (np.arange(n, dtype=np.uint64) // 2).astype(">u8").view(np.uint8)
    recs = np.zeros((n, 4), np.uint64)
    recs[:, 0] = 8 * np.arange(n, dtype=np.uint64)
    recs[:, 1] = 8
    recs[:, 2] = recs[:, 0] + 8
    wres = [0, n_out, n, 0, 8 * n_out, 0, n - n_out, 0]
    assert wres == [0, 524289, 1048577, 0, 8 * 524289, 0, 524288, 0]
    d_src = torch.from_numpy(src).to(gpu)
    perm = np.random.default_rng(5).permutation(n)
    for order in (np.arange(n), perm):
        listed = recs[order]
        # sorted by (key, position in the list): the winner of a key is the last of its run
        key = order // 2
        by_key = np.lexsort((np.arange(n), key))
        last = np.ones(n, bool)
        last[:-1] = key[by_key][1:] != key[by_key][:-1]
        want = listed[by_key[last]]
        assert len(want) == n_out
        if order is not perm:                                  # as listed: the odd i and the last record
            assert np.array_equal(want, recs[np.r_[1:n:2, n - 1]])
        out, res = repack.device_merge(d_src, [(dm.dev_recs(listed, gpu), 0)],
                                       out=torch.zeros((n, 4), dtype=torch.int64, device=gpu))
        assert [int(v) for v in res.cpu().numpy().view(np.uint64)] == wres
        assert np.array_equal(out.cpu().numpy().view(np.uint64)[:n_out], want)


# ------------------------------------------------------------------------ random
@pytest.mark.parametrize("seed", range(20))
def test_random(gpu, seed):
    c = mc.random_case(seed)
    assert c.n == 2000 and 1 <= len(c.lists) <= 4
    dev_in = (dm.dev_bytes(c.src, gpu), [(dm.dev_recs(r, gpu), b) for r, b in c.lists])
    for drop in (False, True):
        _same(c, gpu, drop, tile=(64, 256, 0)[seed % 3], dev_in=dev_in)


# -------------------------------------------------------------------- end to end
def _arena(images, dev):
    """The images one after another at multiples of 64 in one device tensor: (arena, [(off, size)])."""
    buf, at = bytearray(), []
    for img in images:
        buf += bytes(-len(buf) % 64)
        at.append((len(buf), len(img)))
        buf += img
    return dm.dev_bytes(bytes(buf), dev), at


def _finalised_images():
    rng = np.random.default_rng(12)
    images = []
    for idx in range(3, 6):
        w = zf.FileWriter(UUID, idx=idx)
        for t in range(60):
            k = b"%016d" % int(rng.integers(0, 90))
            if t % 7 == 3:
                w.remove(k)
            else:
                w.add(k, rng.integers(0, 256, int(rng.integers(0, 90)), dtype=np.uint8).tobytes())
            w.commit()
        images.append(w.image())
    return images


def _packed_images():
    rng = np.random.default_rng(13)

    def recs(n, lo, hi):
        out = {}
        for _ in range(n):
            k = b"%016d" % int(rng.integers(lo, hi))
            out[k] = None if rng.integers(0, 5) == 0 else rng.integers(0, 256, int(rng.integers(0, 70)),
                                                                     dtype=np.uint8).tobytes()
        return sorted(out.items())
    return zf.packed_file(recs(150, 0, 300), UUID, 4, 7), zf.packed_file(recs(100, 100, 400), UUID, 8, 9)


def test_device_repack_finalised_files(gpu, tmp_path):
    images = _finalised_images()
    merged = zf.repack_finalised(images)
    assert any(v is None for _, v in merged) and len(merged) < 180      # deletes kept, keys overlap
    want = zf.packed_file(merged, UUID, 3, 5)
    arena, at = _arena(images, gpu)
    img, rep = repack.device_repack(arena, at, [zsfile.FINALISED] * 3, UUID, 3, 5, drop_deletes=False)
    assert img.cpu().numpy().tobytes() == want
    assert rep["records_in"] == 180 and rep["records_out"] == len(merged) and rep["deletes_dropped"] == 0
    assert rep["records_out"] + rep["superseded"] == 180 and rep["file_bytes"] == len(want)
    # the same DB on disk through the host repack
    for idx, image in zip(range(3, 6), images):
        (tmp_path / f"zeroskip-{UUIDSTR}-{idx}-{idx}").write_bytes(image)
    (tmp_path / ".zsdb").write_bytes(zf.dotzsdb_bytes(4096, UUIDSTR.encode() + b"\0", 6))
    host = repack.repack_dir(str(tmp_path))
    assert host["branch"] == 1 and (host["startidx"], host["endidx"]) == (3, 5)
    assert open(host["path"], "rb").read() == img.cpu().numpy().tobytes()
    assert host["records_in"] == rep["records_in"] and host["records_out"] == rep["records_out"]


def test_device_repack_packed_files(gpu):
    older, newer = _packed_images()
    merged = zf.repack_packed(older, newer)
    both = set(k for k, _ in zf.packed_records(older)) & set(k for k, _ in zf.packed_records(newer))
    assert both and any(v is None for _, v in zf.packed_records(older))
    want = zf.packed_file(merged, UUID, 4, 9)
    arena, (a_old, a_new) = _arena([older, newer], gpu)
    # the newer file first, the older last: the older wins a key in both
    img, rep = repack.device_repack(arena, [a_new, a_old], [zsfile.PACKED] * 2, UUID, 4, 9, drop_deletes=True)
    assert img.cpu().numpy().tobytes() == want
    assert rep["records_out"] == len(merged) and rep["deletes_dropped"] > 0
    assert rep["records_out"] + rep["superseded"] + rep["deletes_dropped"] == rep["records_in"]
