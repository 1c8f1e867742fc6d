"""zscrc_device_walk and zscrc_device_verify_image at the geometry that ships
(1 MiB blocks, 16 KiB tiles) on images that fill several blocks: a 2.4 MB image
of small records (tests/walk_images.py) well-formed, capped, mutated and at an
unaligned device address; the crafted boundary images built against 1 MiB / 16
KiB and 64 KiB / 4 KiB; zscrc_device_verify_image's second walk and its small
and odd inputs; one image beyond 4 GiB.  The reference is the host walk /
zscrc_zs_verify_image on the same bytes, equal throughout.

What each test is the first to reach (zscrc_walk.hip unless zscrc_zs.cpp is named):

  test_big_wellformed        walk_table_kernel's `rj = a.J[n]; rc = a.C[n] + cm` through up to 63 later
                             tiles of a block; walk_chain_kernel hopping over three full blocks;
                             walk_emit_kernel's `rank = base + ...` with Entry.base > 0 and per = 8 (4, 2)
  test_big_cap               `rank < a.cap` false in one entered block and true in the one before;
                             `n > a.cap` at n == cap (no OVERFLOW) and n == cap + 1
  test_big_fuzz              the chain's S_TRUNC / S_STOP exit with the exit record in block 1 or 2, and
                             the emit kernel's s_cur = NONE part way through those blocks
  test_big_unaligned_...     serial_walk() entered with n > 0 from block 2; res[3] / res[4] folded by the
                             atomics of three blocks over the words the one-lane tail stored
  test_big_boundaries        link_of() / exit_code() at a 1 MiB block edge and a 16 KiB tile edge; a long
                             commit's and a long key's second and third word read from the next block;
                             `cur / a.ts != t` skipping whole 2048-slot tiles
  test_unaligned_base*       be64()'s byte-wise path, for every word of every kernel; the commit kernels
                             under zscrc_device_verify_image on such a base
  test_verify_second_walk    zscrc_zs.cpp: `res[1] <= cap` false -> free, cap = res[1], second pass, and
                             verify_spans() on the second block's arrays
  test_verify_small_and_...  zscrc_zs.cpp: `image_size < HDR`; n == 0 with a block allocated; a STOPPED walk
  test_verify_on_a_stream... hipStreamWaitEvent(s, sc.last) reached from zscrc_device_verify_image
  test_walk_beyond_4gib      `k << 3`, `off - s.span`, be64(img + v + 8) and a long commit's span above
                             2^32; exit_code()'s rel of 2^29 slots; scratch_bytes() above 4 GiB
  tests/test_gpu_walk.py at NEW_GEOMETRIES: `if (i >= a.ts) break` at j = 0 (ts = 16, 32, 128: threads
                             without a slot, `first < a.ts` false in the scan), at j = 1 (ts = 256), j = 2
                             and 4 (per = 2, 4); one tile per block (no later-tile branch at 2048 slots);
                             one block whose `bend` is a.ns"""
import time

import numpy as np
import pytest
import torch

from oracle import zs_format as zf
from tests import devmem as dm
from tests import walk_images as wi
from tests.devmem import CANARY
from tests.images import U64_MAX, UUID, build_active
from tests.walk_images import dev_image as _dev
from tests.walk_images import u64 as _u64
from zeroskip_amd import zsfile
from zeroskip_amd._lib import lib

pytestmark = pytest.mark.gpu

MIB = 1 << 20
# (block_bytes, tile_bytes); 0 = the library's default (1 MiB, 16 KiB)
SCALE_GEOMETRIES = [(0, 0), (1 << 30, 16384), (MIB, 8192), (65536, 4096)]
SCALE_IDS = ["default", "b1g_t16384", "b1m_t8192", "b65536_t4096"]


def _walk(d, cap, block=0, tile=0, serial=False, scratch=None):
    """device_walk into arrays of exactly `cap` entries: (off[:n], len[:n], res) as uint64."""
    off, ln, res = zsfile.device_walk(d, cap=cap, block_bytes=block, tile_bytes=tile, serial=serial, scratch=scratch)
    r = _u64(res)
    n = min(int(r[1]), cap)
    return _u64(off[:n]), _u64(ln[:n]), r


def _equal(host, got, what):
    """Every word of a device walk against the host walk (off, len, rc, end)."""
    hoff, hlen, hrc, hend = host
    off, ln, r = got
    assert (int(r[0]), int(r[1]), int(r[2])) == (hrc, len(hoff), hend), what
    assert np.array_equal(off, hoff) and np.array_equal(ln, hlen), what
    assert int(r[3]) == (int(hlen.max()) if len(hlen) else 0), what
    assert int(r[4]) == (int(hlen.min()) if len(hlen) else 0), what
    return r


def _shifted(img: bytes, shift: int, dev) -> torch.Tensor:
    """img in device memory at an address = shift (mod 8)."""
    buf = torch.empty(len(img) + 16, dtype=torch.uint8, device=dev)
    at = (shift - buf.data_ptr()) % 8
    d = buf[at:at + len(img)]
    d.copy_(torch.from_numpy(np.frombuffer(img, dtype=np.uint8).copy()))
    assert d.data_ptr() % 8 == shift and d.is_contiguous()
    return d


@pytest.fixture(scope="module")
def big():
    """(image, its host walk): three default blocks of small records."""
    img = wi.big_image()
    h = wi.host_walk(img)
    assert h[2:] == (zsfile.END, len(img)) and len(h[0]) > 10000
    return img, h


@pytest.fixture(scope="module")
def d_big(gpu, big):
    return _dev(big[0], gpu)


# ---------------------------------------------------------------- well-formed
@pytest.mark.parametrize("block,tile", SCALE_GEOMETRIES, ids=SCALE_IDS)
def test_big_wellformed(gpu, big, d_big, block, tile):
    img, h = big
    cap = len(img) // 8 + 1
    r = _equal(h, _walk(d_big, cap, block, tile), (block, tile))
    assert int(r[5]) == U64_MAX
    need = zsfile.walk_scratch_bytes(len(img), block, tile)
    assert need > 0
    whole, scratch = dm.fenced(need, gpu)
    assert scratch.data_ptr() % 16 == 0
    r = _equal(h, _walk(d_big, cap, block, tile, scratch=scratch), (block, tile, "caller scratch"))
    assert int(r[5]) == U64_MAX
    assert dm.intact(whole, need)


def test_big_serial_flag(gpu, big, d_big):
    img, h = big
    _equal(h, _walk(d_big, len(h[0]), serial=True), "serial")


# ------------------------------------------------------------------------ cap
def test_big_cap(gpu, big, d_big):
    img, (hoff, hlen, hrc, hend) = big
    n = len(hoff)
    # the commits whose record starts in default block 0: the cut between two entered blocks
    c1 = int(((hoff + hlen) < MIB).sum())
    assert 1000 < c1 < n - 1000
    for cap in (n, n - 1, n + 1, 0, c1 - 1, c1, c1 + 1):
        room = max(cap, 1) * 8
        fo, off = dm.fenced(room, gpu)
        fl, ln = dm.fenced(room, gpu)
        fr, res = dm.fenced(8 * zsfile.WALK_RES_WORDS, gpu)
        zsfile.device_walk(d_big, cap=cap, out=(off.view(torch.int64), ln.view(torch.int64), res.view(torch.int64)))
        r = _u64(res.view(torch.int64))
        assert int(r[0]) == (zsfile.OVERFLOW if cap < n else hrc), cap
        assert (int(r[1]), int(r[2])) == (n, hend), cap
        assert int(r[3]) == int(hlen.max()) and int(r[4]) == int(hlen.min()), cap
        k = min(cap, n)
        assert np.array_equal(_u64(off.view(torch.int64))[:k], hoff[:k]), cap
        assert np.array_equal(_u64(ln.view(torch.int64))[:k], hlen[:k]), cap
        # nothing at or beyond cap (or beyond the commits there are) is touched
        assert bool((off[k * 8:] == CANARY).all()) and bool((ln[k * 8:] == CANARY).all()), cap
        assert dm.intact(fo, room) and dm.intact(fl, room) and dm.intact(fr, 8 * zsfile.WALK_RES_WORDS), cap


# ----------------------------------------------------------------------- fuzz
def test_big_fuzz(gpu):
    """The 120 mutants tests/test_walk_images.py checks the shares and the
    spread of, at the default geometry and with 8 KiB tiles."""
    seen = {zsfile.END: 0, zsfile.STOPPED: 0, zsfile.TRUNCATED: 0}
    for i, m in enumerate(wi.big_fuzz()):
        h = wi.host_walk(m)
        seen[h[2]] += 1
        d = _dev(m, gpu)
        cap = len(h[0]) + 1
        for block, tile in ((0, 0), (MIB, 8192)):
            _equal(h, _walk(d, cap, block, tile), (i, len(m), block, tile))
    assert min(seen.values()) >= 12, seen


def test_big_unaligned_continuation(gpu, big, d_big):
    """The chain's blocks fold their span lengths by atomics, the one-lane
    tail (from the first unaligned offset, in block 2) writes its own."""
    img, first = wi.unaligned_image(big[0])
    h = wi.host_walk(img)
    assert (h[2], h[3], len(h[0])) == (zsfile.END, len(img), len(big[1][0]) + 1) and h[3] % 8 == 4
    assert int(h[1][-1]) == 12 < int(big[1][1].min())  # the tail's span is the shortest: res[4] comes from it
    d = _dev(img, gpu)
    for block, tile in ((0, 0), (MIB, 8192)):
        r = _equal(h, _walk(d, len(h[0]) + 1, block, tile), (block, tile))
        assert int(r[5]) == first


# ------------------------------------------------------------------ boundaries
@pytest.mark.parametrize("B,T", [(MIB, 16384), (65536, 4096)], ids=["b1m_t16384", "b65536_t4096"])
def test_big_boundaries(gpu, B, T):
    """A record, a long commit and a key header across a 1 MiB / 16 KiB (64 KiB
    / 4 KiB) boundary: at the geometry built for, at the default and one-lane."""
    for name, img in wi.boundary_cases(B, T):
        h = wi.host_walk(img)
        d = _dev(img, gpu)
        cap = len(h[0]) + 1
        for block, tile in sorted({(B, T), (MIB, 16384)}):
            r = _equal(h, _walk(d, cap, block, tile), (name, block, tile))
            assert int(r[5]) == U64_MAX, name
        _equal(h, _walk(d, cap, B, T, serial=True), (name, "serial"))


# -------------------------------------------------------------- unaligned base
@pytest.mark.parametrize("shift", [1, 4, 7])
def test_unaligned_base(gpu, big, shift):
    """The image at a device address that is no multiple of 8 (be64()'s
    byte-wise path for every word)."""
    img, h = big
    d = _shifted(img, shift, gpu)
    for block, tile in ((0, 0), (512, 64)):
        r = _equal(h, _walk(d, len(h[0]) + 1, block, tile), (shift, block, tile))
        assert int(r[5]) == U64_MAX
    for name, small in wi.boundary_cases(4096, 512):
        hs = wi.host_walk(small)
        ds = _shifted(small, shift, gpu)
        for block, tile in ((0, 0), (512, 64)):
            _equal(hs, _walk(ds, len(hs[0]) + 1, block, tile), (name, shift, block, tile))


def test_unaligned_base_verify(gpu, big):
    img, h = big
    want = zsfile.verify_image(img, zsfile.ACTIVE)
    assert want["n_commits"] == len(h[0]) and want["n_bad"] == 0 and want["header_rc"] == 0
    for shift in (1, 4, 7):
        got = zsfile.verify_device_image(_shifted(img, shift, gpu), zsfile.ACTIVE)
        assert got == want, (shift, got, want)


# ------------------------------------------------- zscrc_device_verify_image
def _verify_both(img: bytes, kind, dev):
    want = zsfile.verify_image(img, kind)
    got = zsfile.verify_device_image(_dev(img, dev), kind)
    assert got == want, (got, want)
    return got


def test_verify_second_walk(gpu):
    """1000 commits where the first walk has room for 626: the arrays the
    second walk filled are the ones verified."""
    img = wi.dense_commit_image(1000)
    rep = _verify_both(img, zsfile.ACTIVE, gpu)
    assert rep["n_commits"] == 1000 and rep["n_bad"] == 0 and rep["walk_rc"] == zsfile.END
    hoff, hlen, _, _ = wi.host_walk(img)
    b = bytearray(img)
    b[int(hoff[700]) + 5] ^= 0x04                     # a byte of commit 700's span
    b[int(hoff[650] + hlen[650]) + 7] ^= 0x01         # commit 650's stored CRC
    rep = _verify_both(bytes(b), zsfile.ACTIVE, gpu)
    assert rep["n_commits"] == 1000 and rep["n_bad"] == 2 and rep["first_bad"] == 650


def test_verify_small_and_stopped(gpu):
    hdr = zf.header_bytes(UUID, 1, 1)
    rep = _verify_both(hdr[:39], zsfile.ACTIVE, gpu)  # no header, no walk
    assert rep["header_rc"] != 0 and rep["walk_rc"] != 0 and rep["n_commits"] == 0
    rep = _verify_both(hdr, zsfile.ACTIVE, gpu)       # a header alone
    assert (rep["header_rc"], rep["walk_rc"], rep["end_off"], rep["n_commits"]) == (0, zsfile.END, 40, 0)
    # a finalise commit in mid-file: the walk stops there, the commits before it are verified
    w = zf.FileWriter(UUID, idx=7)
    for t in range(40):
        w.add(b"s%05d" % t, b"u" * (t * 11))
        w.commit(final=t == 25)
    img = w.image()
    rep = _verify_both(img, zsfile.ACTIVE, gpu)
    assert rep["walk_rc"] == zsfile.STOPPED and rep["n_commits"] == 25 and rep["n_bad"] == 0
    assert 40 < rep["end_off"] < len(img)
    b = bytearray(img)
    b[60] ^= 0x20                                     # a byte of the first span
    rep = _verify_both(bytes(b), zsfile.ACTIVE, gpu)
    assert rep["walk_rc"] == zsfile.STOPPED and rep["n_bad"] == 1 and rep["first_bad"] == 0


def test_verify_finalised(gpu):
    w = zf.FileWriter(UUID, idx=8)
    for t in range(300):
        w.add(b"f%06d" % t, b"q" * (t % 90))
        if t % 5 == 4:
            w.commit()
    w.add(b"last", b"one")
    w.finalise()
    img = w.image()
    assert len(img) > wi.DEF_TILE
    rep = _verify_both(img, zsfile.FINALISED, gpu)
    assert rep["walk_rc"] == zsfile.END and rep["n_commits"] == 61 and rep["n_bad"] == 0
    b = bytearray(img)
    b[-1] ^= 0x02                                     # the finalising commit's stored CRC
    rep = _verify_both(bytes(b), zsfile.FINALISED, gpu)
    assert rep["n_bad"] == 1 and rep["first_bad"] == 60
    # finalised after a committed transaction: a zero-length commit hashed from the previous span's
    # CRC, which a verifier that starts every commit from 0 rejects (oracle/zs_format.py, finalise)
    w.finalise()
    rep = _verify_both(w.image(), zsfile.FINALISED, gpu)
    assert rep["walk_rc"] == zsfile.END and rep["n_commits"] == 62
    assert rep["n_bad"] == 1 and rep["first_bad"] == 61


def test_verify_on_a_stream_after_a_walk_on_another(gpu, big, d_big):
    """Both use the library's scratch: the verify's walk on stream s must
    wait for the walk enqueued on the default stream just before it."""
    img, h = big
    other = build_active(90, seed=12)
    d_other = _dev(other, gpu)
    want = zsfile.verify_image(img, zsfile.ACTIVE)
    _walk(d_big, len(h[0]))  # the library's scratch is large enough from here on: nothing reallocates below
    torch.cuda.synchronize(gpu)
    s = torch.cuda.Stream(device=gpu)
    off, ln, res = zsfile.device_walk(d_other, block_bytes=512, tile_bytes=64)
    with torch.cuda.stream(s):
        got = zsfile.verify_device_image(d_big, zsfile.ACTIVE)
    torch.cuda.synchronize(gpu)
    assert got == want and got["n_commits"] == len(h[0]) and got["n_bad"] == 0
    ho = wi.host_walk(other)
    r = _u64(res)
    _equal(ho, (_u64(off[:len(ho[0])]), _u64(ln[:len(ho[0])]), r), "the walk on the default stream")


# ------------------------------------------------------------- beyond 4 GiB
def test_walk_beyond_4gib(gpu):
    """Offsets, a value length and a span length above 2^32 (4.0 GiB of
    image, as much scratch): one walk at the default geometry."""
    t0 = time.perf_counter()
    pieces, size = wi.huge_image_pieces()
    a = np.zeros(size, np.uint8)
    n = wi.huge_commits()
    d = torch.zeros(size, dtype=torch.uint8, device=gpu)
    for at, b in pieces:
        a[at:at + len(b)] = np.frombuffer(b, np.uint8)
        d[at:at + len(b)] = torch.from_numpy(np.frombuffer(b, np.uint8).copy()).to(gpu)
    h = wi.host_walk_capped(a, n + 8)
    assert (h[2], h[3], len(h[0])) == (zsfile.END, size, n) and int(h[1].max()) > 1 << 32
    try:
        r = _equal(h, _walk(d, n + 8), "beyond 4 GiB")
        assert int(r[5]) == U64_MAX and int(r[3]) > 1 << 32
    finally:
        del d
        torch.cuda.empty_cache()
        lib().zscrc_release_cache()
    print(f"beyond 4 GiB: {time.perf_counter() - t0:.2f} s")
