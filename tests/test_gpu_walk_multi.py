"""zscrc_device_walk_multi and zscrc_device_verify_images (zeroskip_amd/csrc/
zscrc_walk.hip) against the host walk of each image and the
single-image entry points: k images of one device buffer walked in one call,
spans as offsets into the buffer, a row per image and the totals, equal word
for word; the reports of verify_device_images equal verify_device_image of
each image's own bytes.  Images lie at every residue mod 8 with canary bytes
around them; output arrays are longer than `cap` and checked to be untouched
past what a call may write."""
import random

import numpy as np
import pytest
import torch

from oracle import zs_format as zf
from tests import fuzzlib
from tests import devmem as dm
from tests import walk_images as wi
from tests.arena_cases import arena as _arena
from tests.arena_cases import finalised as _finalised
from tests.arena_cases import key70k as _key70k
from tests.arena_cases import stopped as _stopped
from tests.arena_cases import walk_check as _check
from tests.arena_cases import walk_expect as _expect
from tests.arena_cases import walk_run as _run
from tests.images import U64_MAX, UUID, build_active
from zeroskip_amd import zsfile

pytestmark = pytest.mark.gpu

GEOMETRIES = [(0, 0), (64, 64), (512, 64), (4096, 512), (8192, 1024), (16384, 16384)]
GEOMETRY_IDS = ["default", "b64_t64", "b512_t64", "b4096_t512", "b8192_t1024", "b16384_t16384"]


# ------------------------------------------------------------------ helpers
def _both(images, gaps=None, took_over=None, dev=None):
    buf, descs = _arena(images, gaps)
    return torch.from_numpy(buf).to(dev), descs, _expect(images, descs, took_over)


def _mixed(B: int, T: int):
    """The arena of test_matches_host for blocks of B and tiles of T bytes:
    (images, {index of the unaligned image: the offset its one-lane walk
    starts at})."""
    images = [build_active(200, seed=11)]
    names = []
    for name, img in wi.boundary_cases(B, T):
        names.append(name)
        images.append(img)
    assert {"size_40", "size_47", "final_mid_file", "value_longer_than_two_blocks"} <= set(names)
    images += [b"", zf.header_bytes(UUID, 1, 1)[:39], _finalised()]
    un, first = wi.unaligned_image(build_active(30, seed=2))
    mid = len(images) // 2                 # in the middle: later images' row[6] depends on its counted tail
    images.insert(mid, un)
    return images, {mid: first}


@pytest.fixture(scope="module")
def mixed_default():
    return _mixed(wi.DEF_BLOCK, wi.DEF_TILE)


def _mixed_for(block, tile, mixed_default):
    return mixed_default if block == 0 else _mixed(block, tile)


# -------------------------------------------------------------------- tests
@pytest.mark.parametrize("block,tile", GEOMETRIES, ids=GEOMETRY_IDS)
def test_matches_host(gpu, mixed_default, block, tile):
    images, took = _mixed_for(block, tile, mixed_default)
    d, descs, exp = _both(images, took_over=took, dev=gpu)
    assert sorted({off % 8 for off, _ in descs}) == list(range(8))
    _check(_run(d, descs, block=block, tile=tile), exp, (block, tile))
    (j, first), = took.items()
    rows = exp[3]
    assert int(rows[j][5]) == first and int(rows[j][1]) == 31 and first % 8 == 4
    assert all(int(rows[i][5]) == U64_MAX for i in range(len(rows)) if i != j)
    assert int(rows[j + 1][6]) == int(rows[j][6]) + 31


def test_image_ends_on_commit_then_next_image(gpu):
    short_end = build_active(40, seed=3)
    assert short_end[-8] == zf.REC_COMMIT                   # a short commit is its last 8 bytes
    im = wi.Img()
    im.add(zf.key_record(b"k" * 20) + zf.value_record(b"v" * 333))
    im.add(wi.long_commit(len(im) - 40))
    long_end = im.image()
    assert long_end[-24] == zf.REC_LONG_COMMIT and wi.host_walk(long_end)[2:] == (zsfile.END, len(long_end))
    second = build_active(7, seed=4)
    for first, cuts in ((short_end, (8, 4)), (long_end, (8, 20))):
        for lead in (8, 11):                                # an aligned and an unaligned place
            buf, descs = _arena([first, second], gaps=[lead, 0])
            assert descs[1][0] == descs[0][0] + len(first)  # no byte between the two
            d = torch.from_numpy(buf).to(gpu)
            _check(_run(d, descs), _expect([first, second], descs), "whole")
            _check(_run(d, descs, block=64, tile=64), _expect([first, second], descs), "whole b64")
            for cut in cuts:
                # the same bytes, the first image declared `cut` bytes shorter: the second image's
                # bytes follow its end directly and belong to no record of it
                short = first[:-cut]
                cd = [(descs[0][0], len(short)), descs[1]]
                exp = _expect([short, second], cd)
                if first is long_end or cut == 4:
                    assert int(exp[3][0][0]) == zsfile.TRUNCATED
                assert int(exp[3][0][1]) == len(wi.host_walk(first)[0]) - 1
                _check(_run(d, cd), exp, ("cut", cut))
                _check(_run(d, cd, block=64, tile=64), exp, ("cut b64", cut))


def _fuzz_images():
    """The 600 mutants of tests/test_gpu_walk.py's fuzz_images recipe: the
    same bases, the same random.Random(7)."""
    w = zf.FileWriter(UUID, idx=2)
    for t in range(6):
        for i in range(40):
            w.add(b"%08d" % (t * 100 + i), bytes([i]) * (i * 7 % 200))
        w.commit()
    long_tx = w.image()
    bases = [build_active(30, seed=2), long_tx, _key70k(), _finalised()]
    rng = random.Random(7)
    imgs = []
    while len(imgs) < 600:
        m = fuzzlib.mutate(rng, rng.choice(bases))
        if len(m) > 40:
            imgs.append(m)
    return imgs


def test_fuzz(gpu):
    imgs = _fuzz_images()
    rcs = [wi.host_walk(m)[2] for m in imgs]
    for rc in (zsfile.END, zsfile.STOPPED, zsfile.TRUNCATED):
        share = rcs.count(rc) / len(imgs)
        print(f"host walk result {rc}: {share:.3f} of {len(imgs)} images")
        assert share >= 0.10, (rc, share)
    for a in range(0, len(imgs), 100):
        group = imgs[a:a + 100]
        buf, descs = _arena(group)
        d = torch.from_numpy(buf).to(gpu)
        exp = _expect(group, descs)
        for block, tile in ((512, 64), (0, 0)):
            _check(_run(d, descs, block=block, tile=tile), exp, (a, block, tile))


def test_caps(gpu):
    images = [build_active(20, seed=31), build_active(3, seed=32), b"", build_active(9, seed=33),
              wi.unaligned_image(build_active(6, seed=34))[0], build_active(1, seed=35)]
    took = {4: wi.unaligned_image(build_active(6, seed=34))[1]}
    d, descs, exp = _both(images, took_over=took, dev=gpu)
    total, at3 = exp[4][0], int(exp[3][3][6])
    assert total == 20 + 3 + 9 + 7 + 1 and 1 < at3 < total - 1
    for cap in (1, total - 1, total, total + 1, at3 - 1, at3, at3 + 1, 0):
        for block, tile in ((0, 0), (64, 64)):
            _check(_run(d, descs, cap=cap, block=block, tile=tile), exp, (cap, block))
    _check(_run(d, descs, cap=0, null_arrays=True), exp, "cap 0, no arrays")


def test_unaligned_tail(gpu):
    """A counted tail of four commits that holds its image's (and the arena's)
    shortest and longest span, the image behind it taking its row[6] from the
    tail's count; caps before, inside and at the end of the tail."""
    un, first, n0 = wi.unaligned_tail_image(build_active(30, seed=2))
    images = [build_active(6, seed=31), un, build_active(1, seed=35)]
    d, descs, exp = _both(images, took_over={1: first}, dev=gpu)
    rows, (total, mx, mn) = exp[3], exp[4]
    assert n0 == 30 and total == 6 + 34 + 1
    assert (int(rows[1][1]), int(rows[1][3]), int(rows[1][4])) == (34, mx, mn) and mn == 3
    assert int(rows[2][6]) == int(rows[1][6]) + 34 == 40
    tail = 6 + n0                                           # the index of the tail's first span
    for block, tile in ((0, 0), (64, 64)):
        _check(_run(d, descs, block=block, tile=tile), exp, ("whole", block))
        for cap in (tail - 1, tail, tail + 1, tail + 3, tail + 4, total):
            _check(_run(d, descs, cap=cap, block=block, tile=tile), exp, (cap, block))


def test_order_repeat_overlap(gpu):
    images = [build_active(12, seed=41), build_active(5, seed=42), wi.dense_commit_image(500), build_active(1, seed=43)]
    buf, descs = _arena(images)
    d = torch.from_numpy(buf).to(gpu)
    rev = list(reversed(range(len(images))))
    _check(_run(d, [descs[i] for i in rev]), _expect([images[i] for i in rev], [descs[i] for i in rev]), "reversed")
    order = [2, 0, 2, 1]
    _check(_run(d, [descs[i] for i in order], block=512, tile=64),
           _expect([images[i] for i in order], [descs[i] for i in order]), "repeated")
    # a second descriptor over the first half of an image: the host walk of those bytes
    half = images[2][:len(images[2]) // 2 + 4]
    dd = [descs[2], (descs[2][0], len(half)), descs[0]]
    exp = _expect([images[2], half, images[0]], dd)
    assert int(exp[3][1][0]) == zsfile.TRUNCATED and 0 < int(exp[3][1][1]) < 500
    _check(_run(d, dd), exp, "overlap")
    _check(_run(d, dd, block=64, tile=64), exp, "overlap b64")


def test_many_images(gpu):
    images = [build_active(i % 4, seed=i) for i in range(2000)]
    assert all(40 <= len(m) < 8192 for m in images)      # from a bare header to a few KB
    d, descs, exp = _both(images, dev=gpu)
    assert exp[4][0] == sum(i % 4 for i in range(2000))
    for block, tile in ((0, 0), (64, 64)):
        _check(_run(d, descs, block=block, tile=tile), exp, (block, tile))


def test_multi_block_images(gpu):
    big = wi.big_image()
    images = [build_active(4, seed=51), big, build_active(2, seed=52)]
    d, descs, exp = _both(images, dev=gpu)
    assert len(big) > 2 * wi.DEF_BLOCK
    _check(_run(d, descs), exp, "default")
    skip = dict(wi.boundary_cases(4096, 512))["value_longer_than_two_blocks"]
    images = [_key70k(), skip, build_active(25, seed=53), b"", build_active(3, seed=54)]
    d, descs, exp = _both(images, dev=gpu)
    _check(_run(d, descs, block=4096, tile=512), exp, "b4096")


def test_caller_scratch_fenced(gpu, mixed_default):
    for block, tile in ((0, 0), (512, 64)):
        images, took = _mixed_for(block, tile, mixed_default)
        d, descs, exp = _both(images, took_over=took, dev=gpu)
        need = zsfile.walk_multi_scratch_bytes(descs, block, tile)
        assert need > 0
        whole, scratch = dm.fenced(need, gpu)
        assert scratch.data_ptr() % 16 == 0
        mine = _run(d, descs, block=block, tile=tile, scratch=scratch)
        _check(mine, exp, ("caller scratch", block))
        assert dm.intact(whole, need)
        lib = _run(d, descs, block=block, tile=tile)
        assert all(np.array_equal(a, b) for a, b in zip(mine[:5], lib[:5]))


def test_library_scratch_across_streams(gpu, mixed_default):
    images, took = mixed_default
    d, descs, exp = _both(images, took_over=took, dev=gpu)
    one = build_active(200, seed=11)
    d_one = torch.from_numpy(np.frombuffer(one, dtype=np.uint8).copy()).to(gpu)
    hoff, hlen, hrc, hend = wi.host_walk(one)
    _run(d, descs)                       # the library's scratch is large enough from here on
    torch.cuda.synchronize(gpu)
    side = torch.cuda.Stream(device=gpu)

    def single_ok(res):
        off, ln, r = res
        r = r.cpu().numpy().view(np.uint64)
        assert (int(r[0]), int(r[1]), int(r[2])) == (hrc, len(hoff), hend)
        assert np.array_equal(off[:len(hoff)].cpu().numpy().view(np.uint64), hoff)
        assert np.array_equal(ln[:len(hoff)].cpu().numpy().view(np.uint64), hlen)

    # a single walk on the default stream, the multi-walk on the side stream right behind it
    single = zsfile.device_walk(d_one, block_bytes=512, tile_bytes=64)
    with torch.cuda.stream(side):
        multi = _run(d, descs)
    torch.cuda.synchronize(gpu)
    single_ok(single)
    _check(multi, exp, "multi behind single")
    # and the reverse
    multi = zsfile.device_walk_multi(d, descs)
    with torch.cuda.stream(side):
        single = zsfile.device_walk(d_one, block_bytes=512, tile_bytes=64)
    torch.cuda.synchronize(gpu)
    single_ok(single)
    total = exp[4][0]
    assert np.array_equal(multi[0][:total].cpu().numpy().view(np.uint64), exp[0])
    assert np.array_equal(multi[1][:total].cpu().numpy().view(np.uint64), exp[1])
    assert np.array_equal(multi[2][:total].cpu().numpy().view(np.uint32), exp[2])
    assert np.array_equal(multi[3].cpu().numpy().view(np.uint64), exp[3])


def test_deterministic(gpu, mixed_default):
    images, took = mixed_default
    d, descs, _ = _both(images, took_over=took, dev=gpu)
    a, b = _run(d, descs), _run(d, descs)
    assert all(np.array_equal(x, y) for x, y in zip(a[:5], b[:5]))
    a, b = _run(d, descs, block=4096, tile=512), _run(d, descs, block=4096, tile=512)
    assert all(np.array_equal(x, y) for x, y in zip(a[:5], b[:5]))


# ----------------------------------------------- zscrc_device_verify_images
def _verify_equal(images, dev, gaps=None):
    """verify_device_images of the arena == verify_device_image of each
    image's own slice (and the host's verify_image where the image lies at an
    8-byte aligned offset); returns the reports."""
    buf, descs = _arena(images, gaps)
    d = torch.from_numpy(buf).to(dev)
    got = zsfile.verify_device_images(d, descs)
    assert len(got) == len(images)
    for j, (img, (off, size)) in enumerate(zip(images, descs)):
        want = zsfile.verify_device_image(d[off:off + size], zsfile.ACTIVE)
        assert got[j] == want, (j, got[j], want)
        if off % 8 == 0:
            assert got[j] == zsfile.verify_image(img, zsfile.ACTIVE), j
    return got


def test_verify_images_equals_per_image(gpu):
    good = build_active(50, seed=21)
    base = build_active(40, seed=22)
    hoff, hlen, _, _ = wi.host_walk(base)
    flipped = bytearray(base)
    for c in (0, 20, 39):                                   # a byte inside the first, a middle and the last span
        flipped[int(hoff[c]) + 3] ^= 0x10
    badhdr = bytearray(build_active(10, seed=23))
    badhdr[9] ^= 1                                          # the header's version field
    truncated = good[:len(good) * 2 // 3 + 3]
    images = [good, bytes(flipped), bytes(badhdr), _stopped(), truncated, zf.header_bytes(UUID, 1, 1)[:39],
              _finalised(), build_active(8, seed=24)]
    reps = _verify_equal(images, gpu)
    assert (reps[0]["n_commits"], reps[0]["n_bad"], reps[0]["header_rc"], reps[0]["walk_rc"]) == (50, 0, 0, zsfile.END)
    assert (reps[1]["n_commits"], reps[1]["n_bad"], reps[1]["first_bad"]) == (40, 3, 0)
    assert reps[2]["header_stored"] != reps[2]["header_computed"] and reps[2]["n_bad"] == 0
    assert reps[3]["walk_rc"] == zsfile.STOPPED and reps[3]["n_commits"] == 25
    assert reps[4]["walk_rc"] == zsfile.TRUNCATED and 0 < reps[4]["n_commits"] < 50
    assert reps[5]["header_rc"] != 0 and reps[5]["walk_rc"] < 0 and reps[5]["n_commits"] == 0
    # finalised right after a commit: the zero-length finalise commit chains from the previous span's
    # CRC, which a verifier that starts every commit from 0 rejects (tests/test_gpu_walk_scale.py)
    assert (reps[6]["walk_rc"], reps[6]["n_commits"], reps[6]["n_bad"], reps[6]["first_bad"]) == (zsfile.END, 13, 1, 12)
    # the same at aligned places, where the host's verify_image is the second reference
    _verify_equal(images, gpu, gaps=[8 + 8 * i for i in range(len(images))])
    # first_bad counts within the image: only the last image is bad
    late = bytearray(build_active(8, seed=24))
    o, _, _, _ = wi.host_walk(bytes(late))
    late[int(o[5]) + 1] ^= 0x01
    reps = _verify_equal([good, build_active(3, seed=25), bytes(late)], gpu)
    assert (reps[2]["n_bad"], reps[2]["first_bad"]) == (1, 5) and reps[0]["n_bad"] == reps[1]["n_bad"] == 0


def test_verify_images_second_walk(gpu):
    dense = wi.dense_commit_image(1000)
    images = [build_active(1, seed=61), dense, build_active(2, seed=62)]
    commits = sum(len(wi.host_walk(m)[0]) for m in images)
    assert commits > sum(len(m) // 64 + 1 for m in images)  # the first walk's room does not do
    reps = _verify_equal(images, gpu)
    assert [r["n_commits"] for r in reps] == [1, 1000, 2] and all(r["n_bad"] == 0 for r in reps)
    hoff, hlen, _, _ = wi.host_walk(dense)
    b = bytearray(dense)
    b[int(hoff[700]) + 5] ^= 0x04                           # a byte of commit 700's span
    b[int(hoff[650] + hlen[650]) + 7] ^= 0x01               # commit 650's stored CRC
    reps = _verify_equal([images[0], bytes(b), images[2]], gpu)
    assert (reps[1]["n_commits"], reps[1]["n_bad"], reps[1]["first_bad"]) == (1000, 2, 650)
    assert reps[0]["n_bad"] == 0 and reps[2]["n_bad"] == 0


def test_verify_images_on_side_stream(gpu):
    # (no 0-byte image here: the per-image call has no pointer to be given for one)
    images = [build_active(60, seed=71), wi.dense_commit_image(500), b"\x04", build_active(5, seed=72)]
    buf, descs = _arena(images)
    d = torch.from_numpy(buf).to(gpu)
    want = [zsfile.verify_device_image(d[off:off + size], zsfile.ACTIVE) for off, size in descs]
    other = build_active(90, seed=12)
    d_other = torch.from_numpy(np.frombuffer(other, dtype=np.uint8).copy()).to(gpu)
    zsfile.device_walk_multi(d, descs)   # the library's scratch is large enough from here on
    torch.cuda.synchronize(gpu)
    side = torch.cuda.Stream(device=gpu)
    off, ln, res = zsfile.device_walk(d_other, block_bytes=512, tile_bytes=64)
    with torch.cuda.stream(side):
        got = zsfile.verify_device_images(d, descs)
    torch.cuda.synchronize(gpu)
    assert got == want
    hoff, hlen, hrc, hend = wi.host_walk(other)
    r = res.cpu().numpy().view(np.uint64)
    assert (int(r[0]), int(r[1]), int(r[2])) == (hrc, len(hoff), hend)
    assert np.array_equal(off[:len(hoff)].cpu().numpy().view(np.uint64), hoff)
