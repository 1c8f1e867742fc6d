"""Images for the walk tests (tests/test_gpu_walk.py, tests/test_gpu_walk_scale.py,
tests/test_walk_images.py): crafted records against a block / tile geometry,
a production-scale image of small records, one of back-to-back commits and
the pieces of one larger than 4 GiB.  Every builder checks with the host walk
(zscrc_zs_walk) that its image is what it is meant to be; no GPU is needed."""
import ctypes
import functools
import random
import struct

import numpy as np

from oracle import zs_format as zf
from tests import fuzzlib
from tests.images import UUID, build_active
from zeroskip_amd import zsfile
from zeroskip_amd._lib import lib

T_2ND = zf.REC_2ND_HALF
DEF_BLOCK, DEF_TILE = 1 << 20, 16384

# (block_bytes, tile_bytes) the device walk is run at beyond the default and
# the three toy ones: every power of two of slots per tile from 16 to 2048
NEW_GEOMETRIES = [(128, 128), (1024, 256), (8192, 1024), (65536, 2048), (65536, 4096), (1 << 20, 8192),
                  (16384, 16384), (1 << 30, 16384)]
NEW_GEOMETRY_IDS = ["b128_t128", "b1024_t256", "b8192_t1024", "b65536_t2048", "b65536_t4096", "b1m_t8192",
                    "b16384_t16384", "b1g_t16384"]


def host_walk(img):
    """zsfile.walk as uint64 arrays: (off, len, rc, end)."""
    off, ln, rc, end = zsfile.walk(img)
    return off.astype(np.uint64), ln.astype(np.uint64), rc, end


def dev_image(img: bytes, dev):
    """The image as a device tensor (torch is needed by the GPU tests only)."""
    import torch
    return torch.from_numpy(np.frombuffer(img, dtype=np.uint8).copy()).to(dev)


def u64(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


def device_walk(d, block=0, tile=0, serial=False):
    off, ln, res = zsfile.device_walk(d, block_bytes=block, tile_bytes=tile, serial=serial)
    r = u64(res)
    n = int(r[1])
    return u64(off[:n]), u64(ln[:n]), r


def same_walk(img: bytes, d, block, tile, serial=False):
    """The device walk of d equals the host walk of img; returns its res."""
    hoff, hlen, hrc, hend = host_walk(img)
    off, ln, r = device_walk(d, block, tile, serial)
    what = (len(img), block, tile, serial)
    assert (int(r[0]), int(r[1]), int(r[2])) == (hrc, len(hoff), hend), what
    assert np.array_equal(off, hoff) and np.array_equal(ln, hlen), what
    assert int(r[3]) == (int(hlen.max()) if len(hlen) else 0), what
    assert int(r[4]) == (int(hlen.min()) if len(hlen) else 0), what
    return r


def host_walk_capped(img: np.ndarray, cap: int):
    """zscrc_zs_walk with room for `cap` commits only (zsfile.walk allocates
    size / 8 + 1 entries, 8 GiB for a 4 GiB image)."""
    off = np.empty(cap, np.uint64)
    ln = np.empty(cap, np.uint64)
    nc = ctypes.c_size_t()
    end = ctypes.c_uint64()
    rc = lib().zscrc_zs_walk(img.ctypes.data, img.nbytes, off.ctypes.data, ln.ctypes.data, cap, ctypes.byref(nc),
                             ctypes.byref(end))
    assert rc >= 0 and nc.value <= cap, (rc, nc.value)
    return off[:nc.value], ln[:nc.value], rc, end.value


# ------------------------------------------------------------ crafted images
def short_commit(span_len=0, final=False):
    return zf.be64(((zf.REC_FINAL if final else zf.REC_COMMIT) << 56) | (span_len << 32))


def long_commit(span_len):
    return zf.be64(zf.REC_LONG_COMMIT << 56) + zf.be64(span_len) + zf.be64(T_2ND << 56)


def long_key(key: bytes):
    kbuflen = 24 + zf.rup8(len(key))
    return zf.be64(zf.REC_LONG_KEY << 56) + zf.be64(len(key)) + zf.be64(kbuflen) + key + \
        bytes(kbuflen - 24 - len(key))


class Img:
    """Records laid one after another from the header; pad_to() fills with
    delete records (and 8-byte commits) up to a wanted offset."""

    def __init__(self):
        self.b = bytearray(zf.header_bytes(UUID, 1, 1))

    def __len__(self):
        return len(self.b)

    def add(self, rec: bytes) -> int:
        at = len(self.b)
        self.b += rec
        return at

    def pad_to(self, off: int):
        assert off >= len(self.b) and off % 8 == 0
        while len(self.b) < off:
            gap = off - len(self.b)
            if gap in (8, 16, 32):
                self.b += short_commit(0)
            else:
                self.b += zf.delete_record(bytes([0x41]) * min(gap - 24, 4096))

    def next_at(self, mod: int, rem: int, least: int = 0) -> int:
        """Pad to the next offset == rem (mod `mod`) that leaves `least` bytes
        of ordinary records before it; returns it."""
        self.add(zf.key_record(b"k" * 9) + zf.value_record(b"v" * 21))
        off = len(self.b) + least
        off += (rem - off) % mod
        self.pad_to(off)
        return off

    def image(self) -> bytes:
        return bytes(self.b)


def boundary_cases(B: int, T: int):
    """[(name, image)] against tile T and block B; each case is checked here
    to be what its name says, before any GPU work."""
    out = []

    im = Img()
    a = im.next_at(T, T - 8)
    im.add(short_commit(a - 40))
    b = im.next_at(T, 0)
    im.add(short_commit(8))
    assert a % T == T - 8 and b % T == 0
    out.append(("short_commit_last_and_first_slot", im.image()))

    im = Img()
    a = im.next_at(T, T - 8)
    im.add(long_commit(a - 40))
    b = im.next_at(B, B - 16)
    im.add(long_commit(100))
    im.add(zf.key_record(b"after") + zf.value_record(b"x" * 50) + short_commit(8))
    assert a // T != (a + 23) // T and b // B != (b + 23) // B
    out.append(("long_commit_straddles_tile_and_block", im.image()))

    im = Img()
    a = im.next_at(B, B - 8)
    im.add(zf.key_record(b"K" * 40) + zf.value_record(b"V" * 70) + short_commit(16))
    voff = struct.unpack(">Q", im.b[a:a + 8])[0] & 0xFFFFFFFF
    assert a % B == B - 8 and (a + voff) // B == a // B + 1
    out.append(("key_header_last_slot_of_block", im.image()))

    im = Img()
    a = im.next_at(B, B - 8)
    im.add(long_key(b"L" * 33) + zf.value_record(b"W" * 9) + short_commit(0))
    b = im.next_at(T, T - 16)
    im.add(long_key(b"M" * 8) + zf.value_record(b"") + short_commit(24))
    assert (a + 16) // B == a // B + 1 and (b + 16) // T == b // T + 1
    out.append(("long_key_header_straddles", im.image()))

    im = Img()
    im.add(zf.key_record(b"big") + zf.value_record(bytes(range(256)) * ((2 * B + 300) // 256 + 1)))
    a = im.add(short_commit(64))
    im.add(zf.key_record(b"tail") + zf.value_record(b"t") + short_commit(8))
    assert 40 // B == 0 and a // B >= 2  # the walk enters no block in between
    out.append(("value_longer_than_two_blocks", im.image()))

    im = Img()
    im.next_at(B, B - 8)
    im.add(short_commit(32))
    assert len(im) % B == 0
    out.append(("ends_on_block_boundary", im.image()))

    im = Img()
    im.next_at(T, 8)
    a = im.add(short_commit(16, final=True))
    im.add(zf.key_record(b"never") + zf.value_record(b"seen") + short_commit(8))
    out.append(("final_mid_file", im.image()))
    assert host_walk(im.image())[2:] == (zsfile.STOPPED, a)

    hdr = zf.header_bytes(UUID, 1, 1)
    out.append(("size_40", hdr))
    h = host_walk(hdr)
    assert (len(h[0]), h[2], h[3]) == (0, zsfile.END, 40)
    for extra in range(1, 8):
        img = hdr + bytes([4]) * extra
        h = host_walk(img)
        assert (len(h[0]), h[2], h[3]) == (0, zsfile.TRUNCATED, 40)
        out.append((f"size_{40 + extra}", img))
    return out


def unaligned_image(prefix: bytes):
    """prefix + a key record whose value offset points 28 bytes on, into the
    key's own bytes, at a short value header placed there (offset = 4 mod 8);
    the walk goes on at key + 52, where a commit word stands, and ends at
    key + 60 = the image's end.  Returns (image, first unaligned offset)."""
    assert len(prefix) % 8 == 0
    K = len(prefix)
    key = bytearray(64)
    key[4:12] = zf.be64((zf.REC_VALUE << 56) | (8 << 32))
    key[28:36] = short_commit(12)
    rec = bytearray(zf.key_record(bytes(key)))
    rec[0:8] = zf.be64((zf.REC_KEY << 56) | (64 << 40) | 28)
    img = prefix + bytes(rec[:60])
    assert (K + 28) % 8 == 4 and (K + 52) % 8 == 4
    return img, K + 52


def unaligned_tail_image(prefix: bytes):
    """unaligned_image(prefix) and, behind it, a short commit of span 3, a
    delete record with an 8-byte key, a long commit whose span is len(prefix)
    and a short commit of span 20: every record from the first unaligned
    offset on starts at an offset = 4 mod 8, and the tail the one-lane walk
    takes holds four commits of spans 12, 3, len(prefix) and 20.  Returns
    (image, first unaligned offset, commits before the tail)."""
    img, first = unaligned_image(prefix)
    before = len(host_walk(prefix)[0])
    img += short_commit(3) + zf.delete_record(b"8bytekey") + long_commit(len(prefix)) + short_commit(20)
    assert len(img) == len(prefix) + 132
    off, ln, rc, end = host_walk(img)
    assert (rc, end, len(off)) == (zsfile.END, len(img), before + 4)
    assert [int(v) for v in ln[before:]] == [12, 3, len(prefix), 20] and int(off[before] + ln[before]) == first
    return img, first, before


# ------------------------------------------------------ production-scale images
def small_record_image(min_bytes: int, seed: int) -> bytes:
    """Transactions of 1-3 records (12-byte keys, values of 0-39 bytes), a
    remove in every seventh, until the image exceeds min_bytes: a record
    header in roughly every third 8-byte slot."""
    rng = np.random.default_rng(seed)
    w = zf.FileWriter(UUID, idx=3)
    t = 0
    while len(w.buf) <= min_bytes:
        for _ in range(int(rng.integers(1, 4))):
            k = b"%012d" % int(rng.integers(0, 10**9))
            w.add(k, rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8).tobytes())
        if t % 7 == 3:
            w.remove(b"%012d" % t)
        w.commit()
        t += 1
    return w.image()


BIG_MIN_BYTES = (2 << 20) + (300 << 10)


@functools.lru_cache(maxsize=1)
def big_image() -> bytes:
    """The small-record image every production-scale test uses: three default
    blocks (the last one partly filled), about 170 default tiles."""
    img = small_record_image(BIG_MIN_BYTES, seed=5)
    assert 2 * DEF_BLOCK + 16 * DEF_TILE < len(img) < 3 * DEF_BLOCK
    return img


FUZZ_SEED = 7
FUZZ_COUNT = 120


def big_fuzz():
    """The production-scale fuzz set, one image at a time (120 images of
    2.7 MB are not held together): fuzzlib mutants of big_image()."""
    base = big_image()
    rng = random.Random(FUZZ_SEED)
    n = 0
    while n < FUZZ_COUNT:
        m = fuzzlib.mutate(rng, base)
        if len(m) > 40:
            n += 1
            yield m


def dense_commit_image(n: int) -> bytes:
    """n transactions of one remove and a commit, 40 bytes each: more commits
    than the one per 64 bytes zscrc_device_verify_image's first walk has room
    for, in more than one default tile."""
    w = zf.FileWriter(UUID, idx=6)
    for _ in range(n):
        w.remove(b"k")
        w.commit()
    img = w.image()
    assert len(img) == 40 + 40 * n
    off, _, rc, end = host_walk(img)
    assert (len(off), rc, end) == (n, zsfile.END, len(img))
    assert n > len(img) // 64 + 1, "the first walk's room must not do"
    assert len(img) > DEF_TILE, "the three-launch path at the default geometry"
    return img


HUGE_VALUE = (4 << 30) + (5 << 20)


def huge_image_pieces():
    """([(offset, bytes)], image size) of an image beyond 4 GiB whose other
    bytes are zero: the header; a key whose long value record holds 4 GiB +
    5 MiB of zeros; the records of build_active(30); a long commit whose span
    is everything since the header; a short transaction.  (The walk reads no
    CRC, so none is right here.)"""
    pieces = [(0, zf.header_bytes(UUID, 1, 1))]
    head = zf.key_record(b"huge") + zf.be64(zf.REC_LONG_VALUE << 56) + zf.be64(HUGE_VALUE)
    pieces.append((40, head))
    off = 40 + len(head) + zf.rup8(HUGE_VALUE)
    recs = build_active(30, seed=2)[40:]
    pieces.append((off, recs))
    off += len(recs)
    assert off - 40 > 1 << 32
    pieces.append((off, long_commit(off - 40)))
    off += 24
    tail = zf.key_record(b"tail") + zf.value_record(b"t" * 11)
    tail += short_commit(len(tail))
    pieces.append((off, tail))
    return pieces, off + len(tail)


def huge_commits() -> int:
    """The commits a walk of the huge image finds."""
    return len(host_walk(build_active(30, seed=2))[0]) + 2
