"""What the many-image device tests share (tests/test_gpu_walk_multi.py,
tests/test_gpu_records_multi.py, tests/test_gpu_stages_scale.py): images laid
into one arena with canary bytes around them, what zscrc_device_walk_multi and
zscrc_device_records_multi must give for them from the host walk / the host
lister of each image, the calls into canary-filled arrays longer than `cap`,
and the comparison.  Only GPU tests import this module (it needs torch)."""
import numpy as np
import torch

from oracle import zs_format as zf
from tests import records_images as ri
from tests import walk_images as wi
from tests.devmem import CANARY
from tests.images import U64_MAX, UUID
from zeroskip_amd import zsfile

EINVAL_WORD = U64_MAX                # (uint64_t)(int64_t)ZSCRC_EINVAL
PAD = 64                             # entries behind every output array
CANARY_WORD = int.from_bytes(bytes([CANARY]) * 8, "little")
ROW, TOT = zsfile.RECORDS_ROW_WORDS, zsfile.RECORDS_TOT_WORDS


# ------------------------------------------------------------------- images
def arena(images, gaps=None):
    """The images in one uint8 buffer with canary bytes before, between and
    after them: (buffer, [(off, size)]).  gaps[i] = the canary bytes before
    image i; by default the least number from 8 up that puts image i at an
    offset == i (mod 8), so the offsets take every residue in turn."""
    parts, descs, pos = [], [], 0
    for i, img in enumerate(images):
        gap = gaps[i] if gaps is not None else 8 + (i - pos - 8) % 8
        parts.append(bytes([CANARY]) * gap)
        pos += gap
        assert gaps is not None or pos % 8 == i % 8
        descs.append((pos, len(img)))
        parts.append(bytes(img))
        pos += len(img)
    parts.append(bytes([CANARY]) * 72)
    return np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), descs


def canary(n_bytes: int, dev) -> torch.Tensor:
    return torch.full((n_bytes,), CANARY, dtype=torch.uint8, device=dev)


def finalised() -> bytes:
    w = zf.FileWriter(UUID, idx=5)
    for t in range(12):
        w.add(b"f%04d" % t, b"q" * (t * 13))
        w.commit()
    w.finalise()
    return w.image()


def key70k() -> bytes:
    w = zf.FileWriter(UUID, idx=4)
    w.add(b"a", b"b")
    w.commit()
    w.add(bytes(range(256)) * 273 + b"tail" * 28, b"value of the long key")
    w.commit()
    w.add(b"z", b"")
    w.commit()
    img = w.image()
    assert len(img) > 70000
    return img


def stopped() -> bytes:
    w = zf.FileWriter(UUID, idx=7)
    for t in range(40):
        w.add(b"s%05d" % t, b"u" * (t * 11))
        w.commit(final=t == 25)
    return w.image()


# ----------------------------------------------------------------- the walk
def first_unaligned(img: bytes, rc: int, end: int, n: int) -> int:
    """Row word [5] from the bytes alone: zscrc_zs_walk's loop restated to
    list the offsets it passes (checked here to end as the host walk did);
    the first one that is no multiple of 8 is where a one-lane walk has to
    take over, U64_MAX if there is none."""
    size, off, commits = len(img), 40, 0

    def be64(o):
        return int.from_bytes(img[o:o + 8], "big")

    def rup8(v):
        return (v + 7) & ~7

    def done(code, unaligned=U64_MAX):
        assert (code, off, commits) == (rc, end, n), (code, off, commits, rc, end, n)
        return unaligned

    while off < size:
        if off % 8:
            assert off <= end and commits <= n
            return off                   # the host walk vouches for the rest
        room = size - off
        if room < 8:
            return done(zsfile.TRUNCATED)
        w = be64(off)
        t = w >> 56
        if t in (zf.REC_KEY, zf.REC_LONG_KEY):
            if t == zf.REC_LONG_KEY and room < 24:
                return done(zsfile.TRUNCATED)
            voff = w & 0xFFFFFFFF if t == zf.REC_KEY else be64(off + 16)
            if voff == 0 or voff > room or room - voff < 16:
                return done(zsfile.TRUNCATED)
            v = off + voff
            vw = be64(v)
            vlen = (vw >> 32) & 0xFFFFFF if vw >> 56 == zf.REC_VALUE else be64(v + 8)
            if vlen > size - v - 16 or rup8(vlen) > size - v - 16:
                return done(zsfile.TRUNCATED)
            off = v + 16 + rup8(vlen)
        elif t in (64, 32):              # a delete record, short and long
            if room < 24:
                return done(zsfile.TRUNCATED)
            klen = (w >> 40) & 0xFFFF if t == 64 else be64(off + 8)
            if klen > room - 24 or rup8(klen) > room - 24:
                return done(zsfile.TRUNCATED)
            off += 24 + rup8(klen)
        elif t == zf.REC_COMMIT:
            if (w >> 32) & 0xFFFFFF > off:
                return done(zsfile.TRUNCATED)
            commits += 1
            off += 8
        elif t == zf.REC_LONG_COMMIT:
            if room < 24 or be64(off + 8) > off:
                return done(zsfile.TRUNCATED)
            commits += 1
            off += 24
        else:
            return done(zsfile.STOPPED)
    return done(zsfile.END, off if off % 8 else U64_MAX)


def host_row(img: bytes):
    """(off, len, row words [0..5]) of one image from the host walk."""
    if len(img) < 40:
        z = np.empty(0, np.uint64)
        return z, z, [EINVAL_WORD, 0, 0, 0, 0, U64_MAX]
    off, ln, rc, end = wi.host_walk(img)
    assert rc in (zsfile.END, zsfile.STOPPED, zsfile.TRUNCATED)
    return off, ln, [rc, len(off), end, int(ln.max()) if len(ln) else 0, int(ln.min()) if len(ln) else 0,
                     first_unaligned(bytes(img), rc, end, len(off))]


def walk_expect(images, descs, took_over=None):
    """What the multi-walk must give for these images at these places, from
    the host walk of each: (off, len, img, rows, tot[1..3])."""
    offs, lens, imgs, rows, first = [], [], [], [], 0
    for j, (img, (at, size)) in enumerate(zip(images, descs)):
        assert size == len(img)
        off, ln, row = host_row(img)
        if took_over is not None:        # the builder's own word on where the walk leaves the slots
            assert row[5] == took_over.get(j, U64_MAX), (j, row[5])
        offs.append(off + np.uint64(at))
        lens.append(ln)
        imgs.append(np.full(len(off), j, np.uint32))
        rows.append(row + [first, 0])
        first += len(off)
    ln = np.concatenate(lens)
    tot = [first, int(ln.max()) if first else 0, int(ln.min()) if first else 0]
    return np.concatenate(offs), ln, np.concatenate(imgs), np.array(rows, np.uint64), tot


def walk_run(d_arena, descs, cap=None, block=0, tile=0, scratch=None, null_arrays=False):
    """device_walk_multi into canary-filled arrays PAD entries longer than
    needed; the whole arrays come back as numpy (uint64 / uint32)."""
    dev, k = d_arena.device, len(descs)
    if cap is None:
        cap = sum(size // 8 + 1 for _, size in descs)
    room = 0 if null_arrays else cap + PAD
    out = (canary(8 * room, dev).view(torch.int64), canary(8 * room, dev).view(torch.int64),
           canary(4 * room, dev).view(torch.int32), canary(8 * (8 * k + PAD), dev).view(torch.int64),
           canary(8 * (zsfile.WALK_TOT_WORDS + PAD), dev).view(torch.int64))
    zsfile.device_walk_multi(d_arena, descs, cap=cap, block_bytes=block, tile_bytes=tile, out=out, scratch=scratch)
    off, ln, img, rows, tot = (t.cpu().numpy() for t in out)
    return off.view(np.uint64), ln.view(np.uint64), img.view(np.uint32), rows.view(np.uint64), tot.view(np.uint64), cap


def walk_check(got, exp, what=""):
    off, ln, img, rows, tot, cap = got
    eoff, eln, eimg, erows, (total, mx, mn) = exp
    k = len(erows)
    assert np.array_equal(rows[:8 * k].reshape(k, 8), erows), (what, rows[:8 * k].reshape(k, 8), erows)
    assert [int(v) for v in tot[:4]] == [zsfile.OVERFLOW if total > cap else 0, total, mx, mn], what
    m = min(total, cap)
    assert np.array_equal(off[:m], eoff[:m]) and np.array_equal(ln[:m], eln[:m]), what
    assert np.array_equal(img[:m], eimg[:m]), what
    # nothing at index >= min(total, cap) was written, nor past the rows and the totals
    assert (off[m:] == CANARY_WORD).all() and (ln[m:] == CANARY_WORD).all(), what
    assert (img[m:] == CANARY_WORD & 0xFFFFFFFF).all(), what
    assert (rows[8 * k:] == CANARY_WORD).all() and (tot[4:] == CANARY_WORD).all(), what


# ------------------------------------------------------------- the record lists
def trajectory(img: bytes, h: np.ndarray, rc: int):
    """(row word [2], row word [8]) of an image of 40 bytes and more from its
    host list: the lister's offsets from 40 -- a listed record leads to the
    end of its value (or of its key, a delete), a commit record is 8 or 24
    bytes, anything else is where the lister ended -- and the first of them
    that is no multiple of 8."""
    size, off, i, take = len(img), 40, 0, U64_MAX
    while off < size:
        if off % 8 and take == U64_MAX:
            take = off
        if i < len(h) and int(h[i][0]) == off + 24:
            _, klen, voff, vlen = (int(v) for v in h[i])
            off = off + 24 + zf.rup8(klen) if voff == U64_MAX else voff + zf.rup8(vlen)
            i += 1
            continue
        rl = {zf.REC_COMMIT: 8, zf.REC_LONG_COMMIT: 24}.get(img[off]) if size - off >= 8 else None
        if rl is None or size - off < rl:
            break
        off += rl
    assert i == len(h) and (off == size) == (rc == zsfile.END), (i, len(h), off, size, rc)
    if rc != zsfile.END:
        # the image cut where the lister ended lists the same records and ends there
        ch, crc = ri.host_records(img[:off], zsfile.ACTIVE)
        assert crc == zsfile.END and np.array_equal(ch, h), off
    return off, take


def host_image(img: bytes):
    """(records uint64 [n, 4], row words [0..8]) of one image from the host lister."""
    if len(img) < 40:
        return np.zeros((0, 4), np.uint64), [EINVAL_WORD, 0, 0, 0, 0, 0, 0, 0, U64_MAX]
    h, rc = ri.host_records(bytes(img), zsfile.ACTIVE)
    assert rc in (zsfile.END, zsfile.STOPPED, zsfile.TRUNCATED)
    end, take = trajectory(bytes(img), h, rc)
    return h, [rc, len(h), end] + ri.folds(h) + [take]


def records_expect(images, descs, took_over=None):
    """What the one call must give for these images at these places:
    (recs [n, 4], rows [k, 12], tot[1..7])."""
    recs, rows, first, bad = [], [], 0, 0
    for j, (img, (at, size)) in enumerate(zip(images, descs)):
        assert size == len(img)
        h, row = host_image(img)
        if took_over is not None:        # the builder's own word on where the lister leaves the slots
            assert row[8] == took_over.get(j, U64_MAX), (j, row[8])
        r = h.copy()
        r[:, 0] += np.uint64(at)
        r[r[:, 2] != U64_MAX, 2] += np.uint64(at)
        recs.append(r)
        rows.append(row + [first, 0, 0])
        first += len(h)
        bad += row[0] != zsfile.END
    recs = np.concatenate(recs)
    return recs, np.array(rows, np.uint64), [first] + ri.folds(recs) + [bad]


def records_run(d_arena, descs, cap=None, block=0, tile=0, scratch=None, null_recs=False):
    """device_records_multi into canary-filled arrays PAD entries longer than
    needed; the whole arrays come back as numpy uint64."""
    dev, k = d_arena.device, len(descs)
    if cap is None:
        cap = sum(size // 24 + 1 for _, size in descs)
    room = 0 if null_recs else cap + PAD
    out = (canary(32 * room, dev).view(torch.int64).view(room, 4), canary(8 * (ROW * k + PAD), dev).view(torch.int64),
           canary(8 * (TOT + PAD), dev).view(torch.int64))
    zsfile.device_records_multi(d_arena, descs, cap=cap, block_bytes=block, tile_bytes=tile, out=out, scratch=scratch)
    recs, rows, tot = (t.cpu().numpy().view(np.uint64) for t in out)
    return recs.reshape(room, 4), rows, tot, cap


def records_check(got, exp, what=""):
    recs, rows, tot, cap = got
    erecs, erows, etot = exp
    k, total = len(erows), etot[0]
    assert np.array_equal(rows[:ROW * k].reshape(k, ROW), erows), (what, rows[:ROW * k].reshape(k, ROW), erows)
    assert [int(v) for v in tot[:TOT]] == [zsfile.OVERFLOW if total > cap else 0] + etot, (what, tot[:TOT], etot)
    m = min(total, cap)
    assert np.array_equal(recs[:m], erecs[:m]), what
    # nothing at index >= min(total, cap) was written, nor past the rows and the totals
    assert (recs[m:] == CANARY_WORD).all(), what
    assert (rows[ROW * k:] == CANARY_WORD).all() and (tot[TOT:] == CANARY_WORD).all(), what
