"""Images for the record lister tests (tests/test_records_host.py,
tests/test_gpu_records.py): the files of test_record_lister_matches_oracle, the
three byte patterns on which the lister (zscrc_zs_records) and the walk
(zscrc_zs_walk) disagree, packed files and their mutants.  Every builder
checks on the host that its image is what it is meant to be; no GPU is needed."""
import ctypes
import random
import struct

import numpy as np

from oracle import zs_format as zf
from tests import fuzzlib
from tests.images import U64_MAX, UUID, build_active
from tests.walk_images import Img, short_commit
from zeroskip_amd import repack, zsfile
from zeroskip_amd._lib import lib


def host_records(img: bytes, kind: int):
    """zscrc_zs_records with room for every record: (recs uint64 [n, 4], rc)."""
    cols, rc = repack.records(img, kind)
    return np.ascontiguousarray(cols.T), rc


def host_records_capped(img: bytes, kind: int, cap: int):
    """zscrc_zs_records with room for `cap` records: (recs [min(n, cap), 4], rc, n)."""
    a = np.frombuffer(img, dtype=np.uint8)
    out = np.zeros((max(cap, 1), 4), np.uint64)
    n = ctypes.c_size_t()
    rc = lib().zscrc_zs_records(a.ctypes.data, a.nbytes, kind, out.ctypes.data if cap else None, cap, ctypes.byref(n))
    assert rc >= 0, rc
    return out[:min(n.value, cap)], rc, n.value


def as_pairs(img: bytes, recs) -> list:
    """[(key, value-or-None)] of a record list, as the format oracle gives it."""
    return [(img[a:a + b], None if c == U64_MAX else img[c:c + d]) for a, b, c, d in recs.tolist()]


def finalised_300() -> bytes:
    """The finalised file of test_record_lister_matches_oracle: adds, deletes,
    overwrites, empty values."""
    rng = np.random.default_rng(31)
    w = zf.FileWriter(UUID, idx=4)
    for t in range(300):
        k = b"%016d" % int(rng.integers(0, 90))
        if t % 11 == 3:
            w.remove(k)
        else:
            w.add(k, rng.integers(0, 256, int(rng.integers(0, 700)), dtype=np.uint8).tobytes())
        if t % 3 == 0:
            w.commit()
    w.commit()
    return w.image()


def packed_400(long_value: int = (16 << 20) + 9):
    """(image, records) of test_record_lister_matches_oracle's packed file: 400
    records, every seventh a delete, one value long enough for a long value
    record (more than 2^24 - 1 bytes at the default; a caller that cuts it
    keeps the record but not its long header)."""
    recs = sorted({b"%08d" % i: (None if i % 7 == 1 else bytes([i % 256]) * (i % 50)) for i in range(400)}.items())
    recs[5] = (recs[5][0], b"L" * long_value)
    return zf.packed_file(recs, UUID, 1, 9), recs


def packed_long_value_70k():
    """A 400-record packed file of about 80 KB in which record 5 is a 70 KB
    value behind a LONG value header (written by hand: the writer uses the
    long form only past 16 MiB)."""
    recs = sorted({b"%08d" % i: (None if i % 7 == 1 else bytes([i % 256]) * (i % 50)) for i in range(400)}.items())
    val = b"L" * 70001
    recs[5] = (recs[5][0], val)
    buf = bytearray(zf.header_bytes(UUID, 1, 9))
    ptrs = []
    for i, (key, v) in enumerate(recs):
        ptrs.append(len(buf))
        if v is None:
            buf += zf.delete_record(key)
        elif i == 5:
            buf += zf.key_record(key) + zf.be64(zf.REC_LONG_VALUE << 56) + zf.be64(len(v)) + v + \
                bytes(zf.rup8(len(v)) - len(v))
        else:
            buf += zf.key_record(key) + zf.value_record(v)
    span = len(buf) - 40
    buf += zf.commit_record(0, span)
    pstart = len(buf)
    buf += zf.be64(len(ptrs)) + b"".join(zf.be64(p) for p in ptrs)
    buf += zf.commit_record(0, len(buf) - pstart, final=True)
    img = bytes(buf)
    got, rc = host_records(img, zsfile.PACKED)
    assert rc == 0 and as_pairs(img, got) == recs and img[ptrs[5] + len(zf.key_record(recs[5][0]))] == zf.REC_LONG_VALUE
    return img, recs


def packed_small(n: int):
    """(image, records) of a packed file of n records (n may be 0)."""
    recs = [(b"key%05d" % i, None if i % 5 == 2 else bytes([i]) * (i * 3 % 41)) for i in range(n)]
    img = zf.packed_file(recs, UUID, 2, 4)
    got, rc = host_records(img, zsfile.PACKED)
    assert rc == 0 and as_pairs(img, got) == recs
    return img, recs


def _set_word(img: bytes, at: int, word: int) -> bytes:
    b = bytearray(img)
    b[at:at + 8] = struct.pack(">Q", word)
    return bytes(b)


def packed_crafted(base: bytes):
    """[(name, image)]: the 60-record packed file with one word changed -- a
    pointer that points outside the image, one that points into a value, a
    count larger than the section, a damaged final commit."""
    off, ln, rc = zsfile.packed_spans(base)
    assert rc == 0
    poff, plen = int(off[1]), int(ln[1])
    count = struct.unpack_from(">Q", base, poff)[0]
    assert count == 60 and plen == 8 + 8 * count
    recs, _ = host_records(base, zsfile.PACKED)
    out = [("pointer_outside", _set_word(base, poff + 8 + 8 * 17, len(base) + 4096)),
           ("pointer_far_outside", _set_word(base, poff + 8 + 8 * 3, U64_MAX - 3)),
           ("pointer_at_the_end", _set_word(base, poff + 8 + 8 * 30, len(base) - 4))]
    v = next(i for i in range(count) if recs[i][2] != U64_MAX and recs[i][3] >= 16)
    out.append(("pointer_into_value", _set_word(base, poff + 8 + 8 * (v + 1), int(recs[v][2]))))
    out.append(("count_larger_than_section", _set_word(base, poff, count + 1)))
    out.append(("count_huge", _set_word(base, poff, U64_MAX)))
    out.append(("final_commit_damaged", _set_word(base, len(base) - 8, (zf.REC_FINAL << 56) | (0xFFFFFF << 32))))
    out.append(("final_commit_not_final", _set_word(base, len(base) - 8, (zf.REC_COMMIT << 56) | (plen << 32))))
    # what each does on the host
    want = {"pointer_outside": (zsfile.TRUNCATED, 17), "pointer_far_outside": (zsfile.TRUNCATED, 3),
            "pointer_at_the_end": (zsfile.TRUNCATED, 30), "pointer_into_value": (zsfile.TRUNCATED, v + 1),
            "count_larger_than_section": (zsfile.TRUNCATED, 0), "count_huge": (zsfile.TRUNCATED, 0),
            "final_commit_damaged": (zsfile.TRUNCATED, 0), "final_commit_not_final": (zsfile.TRUNCATED, 0)}
    for name, img in out:
        got, rc = host_records(img, zsfile.PACKED)
        assert (rc, len(got)) == want[name], (name, rc, len(got))
    return out


def packed_mutants(base: bytes, count: int, seed: int = 13):
    """packed_crafted(base) and fuzzlib mutants of base, `count` images of at
    least 56 bytes in all."""
    imgs = [img for _, img in packed_crafted(base)]
    rng = random.Random(seed)
    while len(imgs) < count:
        m = fuzzlib.mutate(rng, base)
        if len(m) >= 56:
            imgs.append(m)
    return imgs


# ------------------------------------------- where the lister and the walk differ
def _tail(im: Img):
    """Ordinary records and a commit behind the crafted one."""
    at = len(im)
    im.add(zf.key_record(b"after-1") + zf.value_record(b"x" * 19))
    im.add(zf.delete_record(b"after-2"))
    im.add(zf.key_record(b"after-3") + zf.value_record(b""))
    im.add(short_commit(len(im) - at))


def commit_span_exceeds_offset():
    """A short commit whose span length exceeds its offset, then more records:
    the walk returns TRUNCATED at it, the lister never looks at the span
    length and goes on.  Returns (image, the commit's offset)."""
    im = Img()
    im.add(zf.key_record(b"before") + zf.value_record(b"v" * 33))
    at = im.add(short_commit(0xFFFFF0))
    _tail(im)
    img = im.image()
    assert 0xFFFFF0 > at
    _, _, rc, end = zsfile.walk(img)
    assert (rc, end) == (zsfile.TRUNCATED, at)
    recs, rc = host_records(img, zsfile.ACTIVE)
    assert rc == zsfile.END and len(recs) == 4
    return img, at


def value_offset_inside_key():
    """A key record with voff = 16, a value header standing there: the walk
    advances over it, the lister returns TRUNCATED.  Returns (image, the
    record's offset)."""
    im = Img()
    im.add(zf.delete_record(b"before"))
    at = im.add(zf.be64((zf.REC_KEY << 56) | (4 << 40) | 16) + zf.be64(0) +
                zf.be64((zf.REC_VALUE << 56) | (8 << 32)) + zf.be64(0) + b"8 bytes.")
    _tail(im)
    img = im.image()
    off, _, rc, end = zsfile.walk(img)
    assert (rc, end, len(off)) == (zsfile.END, len(img), 1)
    recs, rc = host_records(img, zsfile.ACTIVE)
    assert rc == zsfile.TRUNCATED and len(recs) == 1
    return img, at


def key_length_beyond_room():
    """A key record whose klen (65535) exceeds the bytes left but whose value
    offset is valid: the lister returns TRUNCATED, the walk ignores klen.
    Returns (image, the record's offset)."""
    im = Img()
    im.add(zf.key_record(b"before") + zf.value_record(b"v"))
    rec = bytearray(zf.key_record(b"eightkey") + zf.value_record(b"w" * 11))
    rec[0:8] = zf.be64((zf.REC_KEY << 56) | (0xFFFF << 40) | 32)
    at = im.add(bytes(rec))
    _tail(im)
    img = im.image()
    assert len(img) - at < 0xFFFF + 24
    off, _, rc, end = zsfile.walk(img)
    assert (rc, end, len(off)) == (zsfile.END, len(img), 1)
    recs, rc = host_records(img, zsfile.ACTIVE)
    assert rc == zsfile.TRUNCATED and len(recs) == 1
    return img, at


def disagreement_images():
    """[(name, image, offset of the crafted record, the lister's result code)]."""
    a, b, c = commit_span_exceeds_offset(), value_offset_inside_key(), key_length_beyond_room()
    return [("commit_span_exceeds_offset", a[0], a[1], zsfile.END),
            ("value_offset_inside_key", b[0], b[1], zsfile.TRUNCATED),
            ("key_length_beyond_room", c[0], c[1], zsfile.TRUNCATED)]


def wellformed() -> bytes:
    """build_active(200, seed=11): 1-3 adds per transaction, a delete in every
    seventh, more than one default tile."""
    img = build_active(200, seed=11)
    recs, rc = host_records(img, zsfile.ACTIVE)
    assert rc == zsfile.END and len(img) > 16384 and 0 < int((recs[:, 2] == U64_MAX).sum()) < len(recs)
    return img


def folds(h: np.ndarray):
    """res[3..7] of a host record list."""
    if len(h) == 0:
        return [0, 0, 0, 0, 0]
    with np.errstate(over="ignore"):
        return [int((h[:, 2] == U64_MAX).sum()), int(h[:, 1].sum(dtype=np.uint64)), int(h[:, 3].sum(dtype=np.uint64)),
                int(h[:, 1].max()), int(h[:, 3].max())]


def unaligned_records_image(prefix: bytes):
    """prefix + a key record of 4 key bytes whose value offset is 28 (its value
    header right behind the key, at an offset = 4 mod 8) + a delete record, a
    key / value record and a commit, all at offsets = 4 mod 8.  Returns (image,
    the first unaligned offset, the records before the crafted one)."""
    assert len(prefix) % 8 == 0
    K = len(prefix)
    rec = zf.be64((zf.REC_KEY << 56) | (4 << 40) | 28) + bytes(16) + b"key4" + \
        zf.be64((zf.REC_VALUE << 56) | (5 << 32)) + zf.be64(0) + b"value" + bytes(3)
    assert len(rec) == 52
    tail = zf.delete_record(b"8bytekey") + zf.key_record(b"tail-key") + zf.value_record(b"t" * 13)
    img = prefix + rec + tail + short_commit(len(tail))
    before, _ = host_records(prefix, zsfile.ACTIVE)
    h, rc = host_records(img, zsfile.ACTIVE)
    assert rc == zsfile.END and len(h) == len(before) + 3 and (K + 52) % 8 == 4
    assert [int(v) for v in h[len(before)]] == [K + 24, 4, K + 44, 5] and int(h[len(before) + 1][0]) == K + 52 + 24
    return img, K + 52, len(before)
