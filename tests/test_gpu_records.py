"""The device record lister (zscrc_device_records, zeroskip_amd/csrc/zscrc_walk.hip)
against the host lister (zscrc_zs_records / repack.records) on the same bytes,
word for word: the records, the count and the result code; the fold words
res[3..7] computed from the host list; res[2] by a property that needs no
second reference (ACTIVE: the image cut there lists the same records and ends;
PACKED: the pointer section's offset).  Output buffers are canary-filled and
every entry the host would not write must still hold the canary."""
import random

import numpy as np
import pytest
import torch

from oracle import zs_format as zf
from tests import devmem as dm
from tests import fuzzlib
from tests import records_images as ri
from tests.images import U64_MAX, UUID, build_active
from tests.walk_images import boundary_cases, unaligned_image, unaligned_tail_image
from zeroskip_amd import zsfile

pytestmark = pytest.mark.gpu

A, F, P = zsfile.ACTIVE, zsfile.FINALISED, zsfile.PACKED
CANARY64 = 0xA5A5A5A5A5A5A5A5
RES = zsfile.RECORDS_RES_WORDS
# (block_bytes, tile_bytes); 0 = the default; block == tile = 16384; one block for the whole image
GEOMETRIES = [(0, 0), (64, 64), (512, 64), (4096, 512), (16384, 16384), (1 << 30, 16384)]
GEOMETRY_IDS = ["default", "b64_t64", "b512_t64", "b4096_t512", "b16384_t16384", "one_block"]


def _dev(img: bytes, dev, shift: int = 0) -> torch.Tensor:
    """The image in device memory, at an address = shift mod 8."""
    buf = torch.zeros(len(img) + 16, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    d = buf[shift:shift + len(img)]
    d.copy_(torch.from_numpy(np.frombuffer(img, dtype=np.uint8).copy()))
    assert d.data_ptr() % 8 == shift % 8
    return d


def _list(d, kind, cap=None, block=0, tile=0, serial=False, scratch=None):
    """device_records into canary-filled buffers between fences: (recs uint64
    [max(cap, 1), 4], res uint64 [RES])."""
    size = d.numel()
    if cap is None:
        cap = size // 24 + 1
    rows = max(cap, 1)
    fr, recs = dm.fenced(rows * 32, d.device)
    fs, res = dm.fenced(RES * 8, d.device)
    zsfile.device_records(d, kind, cap=cap, block_bytes=block, tile_bytes=tile, serial=serial, scratch=scratch,
                          out=(recs.view(torch.int64).view(rows, 4), res.view(torch.int64)))
    r = res.cpu().numpy().view(np.uint64)
    out = recs.cpu().numpy().view(np.uint64).reshape(rows, 4)
    assert dm.intact(fr, rows * 32) and dm.intact(fs, RES * 8)
    return out, r


def _same(img: bytes, d, kind, host=None, cap=None, what=None, **kw):
    """The device list of d equals the host list of img; returns res."""
    h, hrc = host if host is not None else ri.host_records(img, kind)
    n = len(h)
    full = len(img) // 24 + 1 if cap is None else cap
    got, r = _list(d, kind, cap=cap, **kw)
    what = (what, len(img), kind, cap, kw)
    m = min(n, full)
    assert int(r[0]) == (zsfile.OVERFLOW if n > full else hrc) and int(r[1]) == n, (what, r[:3], hrc, n)
    assert np.array_equal(got[:m], h[:m]), what
    assert bool((got[m:] == CANARY64).all()), what           # nothing stored past min(n, cap)
    assert [int(v) for v in r[3:8]] == ri.folds(h), (what, r[3:8])
    assert [int(v) for v in r[9:12]] == [0, 0, 0], what
    end = int(r[2])
    if kind == P:
        off, _, prc = zsfile.packed_spans(img)
        assert end == (int(off[1]) if prc == 0 else 0), what
        assert int(r[8]) == U64_MAX, what
    else:
        # the image cut where the lister ended lists the same records and ends there
        assert 40 <= end <= len(img) and (end == len(img)) == (hrc == zsfile.END), (what, end)
        ch, crc = ri.host_records(img[:end], kind)
        assert crc == zsfile.END and np.array_equal(ch, h), (what, end)
    return r


@pytest.fixture(scope="module")
def wellformed():
    img = ri.wellformed()
    return img, ri.host_records(img, A)


# ------------------------------------------------------------------ geometries
@pytest.mark.parametrize("block,tile", GEOMETRIES, ids=GEOMETRY_IDS)
def test_wellformed(gpu, wellformed, block, tile):
    img, host = wellformed
    r = _same(img, _dev(img, gpu), A, host, block=block, tile=tile)
    assert int(r[0]) == zsfile.END and int(r[2]) == len(img) and int(r[8]) == U64_MAX
    assert int(r[3]) > 0  # deletes mixed in


def test_serial_flag_and_short_image(gpu, wellformed):
    img, host = wellformed
    d = _dev(img, gpu)
    _same(img, d, A, host, serial=True)
    _same(img, d, F, host, serial=True, block=512, tile=64)
    short = build_active(3, seed=4)
    assert 40 < len(short) < 16384  # less than one default tile: the one-lane kernel
    r = _same(short, _dev(short, gpu), A)
    assert int(r[1]) > 0 and int(r[8]) == U64_MAX
    hdr = zf.header_bytes(UUID, 1, 1)
    for geom in ((0, 0), (64, 64)):
        r = _same(hdr, _dev(hdr, gpu), A, block=geom[0], tile=geom[1])
        assert (int(r[0]), int(r[1]), int(r[2])) == (zsfile.END, 0, 40)


def test_finalised_file_of_the_host_test(gpu):
    img = ri.finalised_300()
    d = _dev(img, gpu)
    for block, tile in ((0, 0), (4096, 512)):
        _same(img, d, F, block=block, tile=tile)


# ------------------------------------------------------------------ boundaries
@pytest.mark.parametrize("B,T", [(512, 64), (4096, 512)], ids=["b512_t64", "b4096_t512"])
def test_boundaries(gpu, B, T):
    for name, img in boundary_cases(B, T):
        d = _dev(img, gpu)
        host = ri.host_records(img, A)
        r = _same(img, d, A, host, what=name, block=B, tile=T)
        assert int(r[8]) == U64_MAX, name
        _same(img, d, A, host, what=name)
        _same(img, d, A, host, what=name, block=B, tile=T, serial=True)


# ------------------------------------------------- where lister and walk differ
@pytest.mark.parametrize("block,tile", [(64, 64), (0, 0)], ids=["b64_t64", "default"])
def test_disagreement_images(gpu, block, tile):
    for name, img, at, want_rc in ri.disagreement_images():
        # (the builders assert what the host walk does with each)
        d = _dev(img, gpu)
        r = _same(img, d, A, what=name, block=block, tile=tile)
        assert int(r[0]) == want_rc, name
        assert int(r[2]) == (len(img) if want_rc == zsfile.END else at), name
        _same(img, d, A, what=name, block=block, tile=tile, serial=True)
    name, img, at, _ = ri.disagreement_images()[0]
    assert zsfile.walk(img)[2:] == (zsfile.TRUNCATED, at)  # the image really separates the two


# ------------------------------------------------------- unaligned continuation
@pytest.mark.parametrize("block,tile", GEOMETRIES[:4], ids=GEOMETRY_IDS[:4])
def test_unaligned_continuation(gpu, wellformed, block, tile):
    """A value offset that is no multiple of 8 leads the lister to records at
    offsets = 4 mod 8: the one-lane loop takes over there (res[8]) and lists
    them, and its folds meet the emit launch's atomics in res[3..7]."""
    prefix, _ = wellformed
    img, first, n0 = ri.unaligned_records_image(prefix)
    host = ri.host_records(img, A)
    d = _dev(img, gpu)
    r = _same(img, d, A, host, block=block, tile=tile)
    assert int(r[8]) == first and int(r[1]) == n0 + 3
    r = _same(img, d, A, host, block=block, tile=tile, serial=True)
    assert int(r[8]) == U64_MAX  # the whole list was the one-lane loop's
    for cap in (n0, n0 + 1, n0 + 2, n0 + 3, n0 + 4):
        r = _same(img, d, A, host, cap=cap, block=block, tile=tile)
        assert int(r[8]) == first
    # the walk tests' unaligned images: their key's value offset (28) lies inside the 64-byte key, so
    # the lister -- unlike the walk -- stops there with TRUNCATED and no loop takes over
    for uimg in (unaligned_image(prefix)[0], unaligned_tail_image(prefix)[0]):
        r = _same(uimg, _dev(uimg, gpu), A, block=block, tile=tile)
        assert (int(r[0]), int(r[2]), int(r[8])) == (zsfile.TRUNCATED, len(prefix), U64_MAX)
        assert zsfile.walk(uimg)[2] == zsfile.END


# ------------------------------------------------------------------------ fuzz
@pytest.fixture(scope="module")
def fuzz_images():
    """600 mutants of the four bases of tests/test_gpu_walk.py's fuzz_images,
    and the host list of each."""
    w = zf.FileWriter(UUID, idx=2)
    for t in range(6):
        for i in range(40):
            w.add(b"%08d" % (t * 100 + i), bytes([i]) * (i * 7 % 200))
        w.commit()
    long_tx = w.image()
    w = zf.FileWriter(UUID, idx=4)
    w.add(b"a", b"b")
    w.commit()
    w.add(bytes(range(256)) * 273 + b"tail" * 28, b"value of the long key")
    w.commit()
    w.add(b"z", b"")
    w.commit()
    key70k = w.image()
    w = zf.FileWriter(UUID, idx=5)
    for t in range(12):
        w.add(b"f%04d" % t, b"q" * (t * 13))
        w.commit()
    w.finalise()
    bases = [build_active(30, seed=2), long_tx, key70k, w.image()]
    rng = random.Random(7)
    imgs = []
    while len(imgs) < 600:
        m = fuzzlib.mutate(rng, rng.choice(bases))
        if len(m) > 40:
            imgs.append(m)
    return [(m, ri.host_records(m, A)) for m in imgs]


def test_fuzz(fuzz_images, gpu):
    seen = {rc: sum(1 for _, h in fuzz_images if h[1] == rc) for rc in (zsfile.END, zsfile.STOPPED, zsfile.TRUNCATED)}
    print("host lister results among the mutants:", seen)
    assert all(seen.values()), seen  # a condition on the inputs: every result code occurs
    for img, host in fuzz_images:
        _same(img, _dev(img, gpu), A, host, block=512, tile=64)


# ------------------------------------------------------------------------- cap
def test_cap(gpu, wellformed):
    img, host = wellformed
    n = len(host[0])
    d = _dev(img, gpu)
    for cap in (n - 2, n - 1, n, n + 1):
        _same(img, d, A, host, cap=cap)
        _same(img, d, A, host, cap=cap, block=4096, tile=512)
        _same(img, d, A, host, cap=cap, serial=True)
    # around the first record of the second block at (4096, 512)
    i0 = int((host[0][:, 0] - 24 < 4096).sum())
    assert 0 < i0 < n - 1
    for cap in (i0 - 1, i0, i0 + 1):
        _same(img, d, A, host, cap=cap, block=4096, tile=512)
    # cap 0: a real array of one entry's room stays untouched; and no array at all (NULL)
    _same(img, d, A, host, cap=0)
    for kw in ({}, {"block_bytes": 4096, "tile_bytes": 512}, {"serial": True}):
        _, res = zsfile.device_records(d, A, cap=0, out=(torch.empty((0, 4), dtype=torch.int64, device=gpu),
                                                         torch.empty(RES, dtype=torch.int64, device=gpu)), **kw)
        r = res.cpu().numpy().view(np.uint64)
        assert (int(r[0]), int(r[1]), int(r[2])) == (zsfile.OVERFLOW, n, len(img))
        assert [int(v) for v in r[3:8]] == ri.folds(host[0])


# -------------------------------------------------------------- device address
@pytest.mark.parametrize("shift", [1, 4, 7])
def test_device_address(gpu, wellformed, shift):
    img, host = wellformed
    d = _dev(img, gpu, shift)
    _same(img, d, A, host)
    _same(img, d, A, host, block=512, tile=64)
    pimg, _ = ri.packed_small(60)
    _same(pimg, _dev(pimg, gpu, shift), P)


# ---------------------------------------------------------------------- packed
def test_packed_400_with_a_long_value_record(gpu):
    img, recs = ri.packed_long_value_70k()  # the 16 MiB + 9 value cut to 70 KB, its long header kept
    d = _dev(img, gpu)
    r = _same(img, d, P)
    assert (int(r[0]), int(r[1])) == (0, 400) and int(r[7]) == 70001
    _same(img, d, P, serial=True)
    for cap in (0, 5, 6, 399, 400, 401):
        _same(img, d, P, cap=cap)
    got, _ = _list(d, P)
    assert ri.as_pairs(img, got[:400]) == recs


def test_packed_without_records(gpu):
    img, _ = ri.packed_small(0)
    r = _same(img, _dev(img, gpu), P)
    assert (int(r[0]), int(r[1])) == (0, 0)
    _, res = zsfile.device_records(_dev(img, gpu), P, cap=0, out=(torch.empty((0, 4), dtype=torch.int64, device=gpu),
                                                                 torch.empty(RES, dtype=torch.int64, device=gpu)))
    assert [int(v) for v in res.cpu().numpy()[:2]] == [0, 0]


@pytest.fixture(scope="module")
def packed_fuzz():
    base, _ = ri.packed_small(60)
    imgs = ri.packed_mutants(base, 200)
    return [(m, ri.host_records(m, P)) for m in imgs]


def test_packed_mutants(packed_fuzz, gpu):
    """The first-failing-pointer rule: res[1] is the host's count, and the
    entries from it on still hold the canary."""
    seen = {}
    for img, host in packed_fuzz:
        key = (host[1], len(host[0]) > 0)
        seen[key] = seen.get(key, 0) + 1
    print("host lister (result, any record listed) among the packed mutants:", seen)
    # well-formed ones, ones cut short part-way through the pointers, ones whose sections are not found
    assert seen.get((0, True)) and seen.get((zsfile.TRUNCATED, True)) and seen.get((zsfile.TRUNCATED, False)), seen
    for img, host in packed_fuzz:
        _same(img, _dev(img, gpu), P, host)


# ---------------------------------------------------------- scratch and streams
@pytest.mark.parametrize("block,tile", [(0, 0), (512, 64)], ids=["default", "b512_t64"])
def test_caller_scratch_fenced(gpu, wellformed, block, tile):
    img, host = wellformed
    need = zsfile.records_scratch_bytes(len(img), A, block, tile)
    assert need > 0
    whole, scratch = dm.fenced(need, gpu)
    assert scratch.data_ptr() % 16 == 0
    _same(img, _dev(img, gpu), A, host, block=block, tile=tile, scratch=scratch)
    assert dm.intact(whole, need)
    pimg, _ = ri.packed_small(60)
    need = zsfile.records_scratch_bytes(len(pimg), P)
    whole, scratch = dm.fenced(need, gpu)
    _same(pimg, _dev(pimg, gpu), P, scratch=scratch)
    assert dm.intact(whole, need)


def test_library_scratch_across_streams(gpu, wellformed):
    """device_walk on the default stream, then device_records on a side stream:
    both use the library's scratch, ordered by its event."""
    img, host = wellformed
    d = _dev(img, gpu)
    hoff, hlen, hrc, hend = zsfile.walk(img)
    side = torch.cuda.Stream(device=gpu)
    torch.cuda.synchronize(gpu)
    off, ln, wres = zsfile.device_walk(d, block_bytes=4096, tile_bytes=512)
    with torch.cuda.stream(side):
        recs, res = zsfile.device_records(d, A, block_bytes=4096, tile_bytes=512)
    torch.cuda.synchronize(gpu)
    w = wres.cpu().numpy()
    assert (int(w[0]), int(w[1]), int(w[2])) == (hrc, len(hoff), hend)
    assert np.array_equal(off[:len(hoff)].cpu().numpy().view(np.uint64), hoff.astype(np.uint64))
    assert np.array_equal(ln[:len(hoff)].cpu().numpy().view(np.uint64), hlen.astype(np.uint64))
    r = res.cpu().numpy().view(np.uint64)
    assert (int(r[0]), int(r[1]), int(r[2])) == (host[1], len(host[0]), len(img))
    assert np.array_equal(recs[:len(host[0])].cpu().numpy().view(np.uint64), host[0])
    assert [int(v) for v in r[3:8]] == ri.folds(host[0])


def test_two_runs_bit_for_bit(gpu, wellformed):
    img, _ = wellformed
    d = _dev(img, gpu)
    for kw in ({}, {"block": 512, "tile": 64}):
        a = _list(d, A, **kw)
        b = _list(d, A, **kw)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    pimg, _ = ri.packed_small(60)
    dp = _dev(pimg, gpu)
    a, b = _list(dp, P), _list(dp, P)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
