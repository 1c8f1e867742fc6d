"""The device walk (zscrc_device_walk, zeroskip_amd/csrc/zscrc_walk.hip) and
zscrc_device_verify_image against the host walk / zscrc_zs_verify_image on
the same bytes: spans, count, result code and end offset equal, at the default
geometry and at blocks / tiles small enough that every boundary case occurs
inside a few KiB; the well-formed, boundary, continuation, cap and scratch
tests at every other number of slots per tile too (tests/walk_images.py,
NEW_GEOMETRIES).  Images of several default blocks: tests/test_gpu_walk_scale.py."""
import random

import numpy as np
import pytest
import torch

from oracle import zs_format as zf
from tests import devmem as dm
from tests import fuzzlib
from tests.devmem import CANARY
from tests.images import U64_MAX, UUID, build_active
from tests.walk_images import (NEW_GEOMETRIES, NEW_GEOMETRY_IDS, Img, boundary_cases, long_commit,  # noqa: F401
                               long_key, short_commit, unaligned_image, unaligned_tail_image)
from tests.walk_images import dev_image as _dev
from tests.walk_images import device_walk as _device
from tests.walk_images import host_walk as _host
from tests.walk_images import same_walk as _same
from tests.walk_images import u64 as _u64
from zeroskip_amd import zsfile

pytestmark = pytest.mark.gpu

# (block_bytes, tile_bytes); 0 = the library's default
OPTSETS = [(0, 0), (64, 64), (512, 64), (4096, 512)]
OPT_IDS = ["default", "b64_t64", "b512_t64", "b4096_t512"]
SMALL = OPTSETS[1:]
# with every other number of slots per tile, block == tile and one block for the whole image
GEOMETRIES = OPTSETS + NEW_GEOMETRIES
GEOMETRY_IDS = OPT_IDS + NEW_GEOMETRY_IDS


@pytest.fixture(scope="module")
def wellformed():
    return build_active(200, seed=11)


# --------------------------------------------------------------------- tests
@pytest.mark.parametrize("block,tile", GEOMETRIES, ids=GEOMETRY_IDS)
def test_wellformed(gpu, wellformed, block, tile):
    img = wellformed
    assert len(img) > 16384  # more than one default tile: the three-launch path at the default too
    r = _same(img, _dev(img, gpu), block, tile)
    assert int(r[0]) == zsfile.END and int(r[1]) == 200
    assert int(r[5]) == U64_MAX


@pytest.fixture(scope="module")
def fuzz_images():
    """600 mutated images and the host walk of each."""
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
    assert len(key70k) > 70000
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
    return [(m, _host(m)) for m in imgs]


def test_fuzz(fuzz_images, gpu):
    # the three outcomes each make up a fair share, from the host walk alone
    for rc in (zsfile.END, zsfile.STOPPED, zsfile.TRUNCATED):
        share = sum(1 for _, h in fuzz_images if h[2] == rc) / len(fuzz_images)
        print(f"host walk result {rc}: {share:.3f} of {len(fuzz_images)} images")
        assert share >= 0.10, (rc, share)
    for img, (hoff, hlen, hrc, hend) in fuzz_images:
        d = _dev(img, gpu)
        for block, tile in OPTSETS:
            off, ln, r = _device(d, block, tile)
            assert (int(r[0]), int(r[1]), int(r[2])) == (hrc, len(hoff), hend), (len(img), block, tile)
            assert np.array_equal(off, hoff) and np.array_equal(ln, hlen), (len(img), block, tile)


@pytest.mark.parametrize("B,T", SMALL, ids=OPT_IDS[1:])
def test_boundaries(gpu, B, T):
    for name, img in boundary_cases(B, T):
        d = _dev(img, gpu)
        for block, tile in GEOMETRIES:
            r = _same(img, d, block, tile)
            assert int(r[5]) == U64_MAX, name
            _same(img, d, block, tile, serial=True)


@pytest.mark.parametrize("block,tile", GEOMETRIES, ids=GEOMETRY_IDS)
def test_unaligned_continuation(gpu, wellformed, block, tile):
    img, first = unaligned_image(wellformed)
    hoff, hlen, hrc, hend = _host(img)
    assert (hrc, hend, len(hoff)) == (zsfile.END, len(img), 201) and hend % 8 == 4
    d = _dev(img, gpu)
    r = _same(img, d, block, tile)
    assert int(r[5]) == first
    r = _same(img, d, block, tile, serial=True)
    assert int(r[5]) == U64_MAX  # the whole walk was the one-lane one


@pytest.mark.parametrize("block,tile", GEOMETRIES, ids=GEOMETRY_IDS)
def test_cap(gpu, wellformed, block, tile):
    img = wellformed
    hoff, hlen, hrc, hend = _host(img)
    n = len(hoff)
    d = _dev(img, gpu)
    for cap in (n // 2, 0):
        # cap 0 too gets real arrays (one entry's room): nothing may be stored there
        room = max(cap, 1) * 8
        fo, off = dm.fenced(room, gpu)
        fl, ln = dm.fenced(room, gpu)
        fr, res = dm.fenced(8 * zsfile.WALK_RES_WORDS, gpu)
        assert off.data_ptr() and ln.data_ptr()
        zsfile.device_walk(d, cap=cap, block_bytes=block, tile_bytes=tile,
                           out=(off.view(torch.int64), ln.view(torch.int64), res.view(torch.int64)))
        r = _u64(res.view(torch.int64))
        assert int(r[0]) == zsfile.OVERFLOW and int(r[1]) == n and int(r[2]) == hend
        assert int(r[3]) == int(hlen.max()) and int(r[4]) == int(hlen.min())
        assert np.array_equal(_u64(off.view(torch.int64))[:cap], hoff[:cap])
        assert np.array_equal(_u64(ln.view(torch.int64))[:cap], hlen[:cap])
        if cap == 0:  # the entry the arrays have room for is untouched
            assert bool((off == CANARY).all()) and bool((ln == CANARY).all())
        assert dm.intact(fo, room) and dm.intact(fl, room) and dm.intact(fr, 8 * zsfile.WALK_RES_WORDS)
    # cap 0 with no arrays at all (the pointers may be NULL then)
    _, _, res = zsfile.device_walk(d, cap=0, block_bytes=block, tile_bytes=tile,
                                   out=(torch.empty(0, dtype=torch.int64, device=gpu),
                                        torch.empty(0, dtype=torch.int64, device=gpu),
                                        torch.empty(zsfile.WALK_RES_WORDS, dtype=torch.int64, device=gpu)))
    r = _u64(res)
    assert int(r[0]) == zsfile.OVERFLOW and int(r[1]) == n and int(r[2]) == hend


@pytest.mark.parametrize("block,tile", GEOMETRIES, ids=GEOMETRY_IDS)
def test_unaligned_tail(gpu, wellformed, block, tile):
    """A tail of four commits behind the first unaligned offset, the image's
    shortest and longest span among them: the one-lane walk's stores, its `cap`
    and its res[3] / res[4], which meet the emit launch's atomics there."""
    img, first, n0 = unaligned_tail_image(wellformed)
    hoff, hlen, hrc, hend = _host(img)
    n = len(hoff)
    assert (hrc, hend, n, n0) == (zsfile.END, len(img), 204, 200)
    assert int(hlen.max()) == int(hlen[n0 + 2]) and int(hlen.min()) == int(hlen[n0 + 1])
    d = _dev(img, gpu)
    r = _same(img, d, block, tile)
    assert int(r[5]) == first
    for cap in (n0 - 1, n0, n0 + 1, n0 + 3, n0 + 4, n0 + 5):
        fo, off = dm.fenced(cap * 8, gpu)
        fl, ln = dm.fenced(cap * 8, gpu)
        fr, res = dm.fenced(8 * zsfile.WALK_RES_WORDS, gpu)
        zsfile.device_walk(d, cap=cap, block_bytes=block, tile_bytes=tile,
                           out=(off.view(torch.int64), ln.view(torch.int64), res.view(torch.int64)))
        r = _u64(res.view(torch.int64))
        what = (cap, block, tile)
        assert int(r[0]) == (zsfile.OVERFLOW if cap < n else zsfile.END), what
        assert (int(r[1]), int(r[2]), int(r[5])) == (n, hend, first), what
        assert int(r[3]) == int(hlen.max()) and int(r[4]) == int(hlen.min()), what
        m = min(cap, n)
        assert np.array_equal(_u64(off.view(torch.int64))[:m], hoff[:m]), what
        assert np.array_equal(_u64(ln.view(torch.int64))[:m], hlen[:m]), what
        # room past the last span (cap n + 1) stays untouched
        assert bool((off[8 * m:] == CANARY).all()) and bool((ln[8 * m:] == CANARY).all()), what
        assert dm.intact(fo, cap * 8) and dm.intact(fl, cap * 8) and dm.intact(fr, 8 * zsfile.WALK_RES_WORDS), what


def test_serial_flag_on_wellformed(gpu, wellformed):
    _same(wellformed, _dev(wellformed, gpu), 0, 0, serial=True)


@pytest.mark.parametrize("block,tile", GEOMETRIES, ids=GEOMETRY_IDS)
def test_caller_scratch_fenced(gpu, wellformed, block, tile):
    img = wellformed
    hoff, hlen, hrc, hend = _host(img)
    need = zsfile.walk_scratch_bytes(len(img), block, tile)
    assert need > 0
    whole, scratch = dm.fenced(need, gpu)
    assert scratch.data_ptr() % 16 == 0
    off, ln, res = zsfile.device_walk(_dev(img, gpu), block_bytes=block, tile_bytes=tile, scratch=scratch)
    r = _u64(res)
    assert (int(r[0]), int(r[1]), int(r[2])) == (hrc, len(hoff), hend)
    assert np.array_equal(_u64(off[:len(hoff)]), hoff) and np.array_equal(_u64(ln[:len(hoff)]), hlen)
    assert dm.intact(whole, need)


def test_scratch_bytes_bound(gpu):
    # 8 bytes per 8-byte slot and 16 per block: <= image_size + 24 * blocks
    for block, tile in OPTSETS:
        bb = block or (1 << 20)
        last = 0
        for size in list(range(40, 300)) + [4095, 4096, 4097, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 5 << 30,
                                            (32 << 30) + 3]:
            need = zsfile.walk_scratch_bytes(size, block, tile)
            blocks = (size + bb - 1) // bb
            if blocks >= 1 << 24:  # more blocks than one launch has workgroups for: a bad option
                assert need == 0, (size, block, tile)
                continue
            assert last <= need <= size + 24 * blocks, (size, block, tile)
            last = need
    assert zsfile.walk_scratch_bytes(1 << 20, 96, 64) == 0     # not a power of two
    assert zsfile.walk_scratch_bytes(1 << 20, 64, 128) == 0    # tile > block
    assert zsfile.walk_scratch_bytes(1 << 20, 1 << 20, 32) == 0


def _verify_both(img: bytes, kind, dev):
    want = zsfile.verify_image(img, kind)
    got = zsfile.verify_device_image(_dev(img, dev), kind)
    assert got == want, (got, want)
    return got


def test_verify_device_image_active(gpu, wellformed):
    img = wellformed
    rep = _verify_both(img, zsfile.ACTIVE, gpu)
    assert rep["n_commits"] == 200 and rep["n_bad"] == 0 and rep["header_rc"] == 0
    hoff, hlen, _, _ = _host(img)
    b = bytearray(img)
    b[int(hoff[57]) + 3] ^= 0x10                      # a payload byte of commit 57's span
    rep = _verify_both(bytes(b), zsfile.ACTIVE, gpu)
    assert rep["n_bad"] == 1 and rep["first_bad"] == 57
    b = bytearray(img)
    b[int(hoff[120] + hlen[120]) + 7] ^= 0x01         # commit 120's stored CRC
    b[int(hoff[33] + hlen[33]) + 6] ^= 0x80
    rep = _verify_both(bytes(b), zsfile.ACTIVE, gpu)
    assert rep["n_bad"] == 2 and rep["first_bad"] == 33
    rep = _verify_both(img[:len(img) * 2 // 3 + 3], zsfile.ACTIVE, gpu)
    assert rep["walk_rc"] == zsfile.TRUNCATED and 0 < rep["n_commits"] < 200
    b = bytearray(img)
    b[9] ^= 1                                         # the header's version field
    rep = _verify_both(bytes(b), zsfile.FINALISED, gpu)
    assert rep["header_stored"] != rep["header_computed"]


def test_verify_device_image_packed(gpu):
    recs = sorted((b"%016d" % i, None if i % 11 == 0 else b"y" * (i % 300)) for i in range(5000))
    img = zf.packed_file(recs, UUID, 2, 9)
    rep = _verify_both(img, zsfile.PACKED, gpu)
    assert rep["walk_rc"] == 0 and rep["n_commits"] == 2 and rep["n_bad"] == 0
    b = bytearray(img)
    b[-8] = zf.REC_COMMIT                             # the final commit word: no longer FINAL
    rep = _verify_both(bytes(b), zsfile.PACKED, gpu)
    assert rep["walk_rc"] == zsfile.TRUNCATED and rep["n_commits"] == 0
    b = bytearray(img)
    b[-1] ^= 0x40                                     # its stored CRC
    rep = _verify_both(bytes(b), zsfile.PACKED, gpu)
    assert rep["n_bad"] == 1 and rep["first_bad"] == 1


def test_verify_device_image_long_commit(gpu):
    w = zf.FileWriter(UUID)
    w.add(b"k" * 100, np.random.default_rng(3).integers(0, 256, (17 << 20) + 5, dtype=np.uint8).tobytes())
    w.commit()
    w.add(b"small", b"v")
    w.commit()
    img = w.image()
    rep = _verify_both(img, zsfile.ACTIVE, gpu)
    assert rep["n_commits"] == 2 and rep["n_bad"] == 0
    # the default geometry's chain skips sixteen blocks here
    r = _same(img, _dev(img, gpu), 0, 0)
    assert int(r[3]) > 17 << 20


def test_back_to_back_on_a_stream(gpu, wellformed):
    a = wellformed
    b = build_active(90, seed=12)
    da, db = _dev(a, gpu), _dev(b, gpu)
    torch.cuda.synchronize(gpu)
    s = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(s):
        ra = zsfile.device_walk(da, block_bytes=4096, tile_bytes=512)
        rb = zsfile.device_walk(db, block_bytes=512, tile_bytes=64)
    s.synchronize()
    for img, (off, ln, res) in ((a, ra), (b, rb)):
        hoff, hlen, hrc, hend = _host(img)
        r = _u64(res)
        assert (int(r[0]), int(r[1]), int(r[2])) == (hrc, len(hoff), hend)
        assert np.array_equal(_u64(off[:len(hoff)]), hoff) and np.array_equal(_u64(ln[:len(hoff)]), hlen)
