"""Record lists for the device packer's tests (tests/test_pack_layout.py on the
CPU, tests/test_gpu_pack_device.py on the GPU): a source blob, a [n, 4] record
list into it (key_off, key_len, val_off or 2^64-1, val_len) and the packed file
it must give.  Every builder checks on the host that its list has the property
it is there for; no GPU is needed."""
import os

import numpy as np

from oracle import oracle
from oracle import zs_format as zf
from tests import records_images as ri
from tests.images import REF as GOLDEN
from tests.images import U64_MAX, UUID
from zeroskip_amd import repack, zsfile


class Case:
    def __init__(self, name, src, recs, want=None, uuid=UUID, startidx=2, endidx=9):
        self.name, self.src, self.uuid, self.startidx, self.endidx = name, bytes(src), uuid, startidx, endidx
        self.recs = np.ascontiguousarray(np.asarray(recs, dtype=np.uint64).reshape(-1, 4))
        self._want = want

    def pairs(self):
        return ri.as_pairs(self.src, self.recs)

    @property
    def want(self) -> bytes:
        if self._want is None:
            self._want = packed_file(self.pairs(), self.uuid, self.startidx, self.endidx)
        return self._want


def long_delete_record(key: bytes) -> bytes:
    """The host packer's delete of a key above 65,535 bytes: the reference
    leaves the first word unwritten (zscrc_pack.cpp, zscrc_pack_add)."""
    assert len(key) > zf.MAX_SHORT_KEY_LEN
    return zf.be64(0) + zf.be64(len(key)) + zf.be64(0) + key + bytes(zf.rup8(len(key)) - len(key))


def packed_file(pairs, uuid, startidx, endidx) -> bytes:
    """zf.packed_file, with the host packer's long delete where the oracle refuses one."""
    if not any(v is None and len(k) > zf.MAX_SHORT_KEY_LEN for k, v in pairs):
        return zf.packed_file(pairs, uuid, startidx, endidx)
    buf = bytearray(zf.header_bytes(uuid, startidx, endidx))
    ptrs = []
    for k, v in pairs:
        ptrs.append(len(buf))
        if v is None:
            buf += long_delete_record(k) if len(k) > zf.MAX_SHORT_KEY_LEN else zf.delete_record(k)
        else:
            buf += zf.key_record(k) + zf.value_record(v)
    span = bytes(buf[40:])
    buf += zf.commit_record(oracle.crc32c_hw(0, span), len(span))
    p = len(buf)
    buf += zf.be64(len(ptrs)) + b"".join(zf.be64(q) for q in ptrs)
    buf += zf.commit_record(oracle.crc32c_hw(0, bytes(buf[p:])), len(buf) - p, final=True)
    return bytes(buf)


class Blob:
    """A source blob built piece by piece, each at a chosen offset mod 16."""

    def __init__(self, seed=0):
        self.buf = bytearray()
        self.rng = np.random.default_rng(seed)

    def put(self, n_or_bytes, residue=None):
        data = self.rng.integers(1, 256, n_or_bytes, dtype=np.uint8).tobytes() if isinstance(n_or_bytes, int) \
            else n_or_bytes
        if residue is not None:
            self.buf += b"\xEE" * ((residue - len(self.buf)) % 16)
        at = len(self.buf)
        self.buf += data
        return at


def from_pairs(name, pairs, seed=0, **kw):
    """Keys and values laid one after another into a blob."""
    b, recs = Blob(seed), []
    for k, v in pairs:
        ko = b.put(k)
        recs.append((ko, len(k), U64_MAX, 0) if v is None else (ko, len(k), b.put(v), len(v)))
    b.put(b"\xEE" * 3)
    return Case(name, b.buf, recs, **kw)


def from_lengths(name, lens, seed=0):
    """(key length, value length or None) pairs, random bytes."""
    b, recs = Blob(seed), []
    for kl, vl in lens:
        ko = b.put(kl)
        recs.append((ko, kl, U64_MAX, 0) if vl is None else (ko, kl, b.put(vl), vl))
    return Case(name, b.buf, recs)


def alignment_grid():
    """Key lengths 0..17 x value lengths 0..17 and a delete, each at every key
    and value source offset mod 16: 18 * 19 * 16 = 5,472 records."""
    b, recs = Blob(5), []
    for r in range(16):
        for kl in range(18):
            for vl in [None] + list(range(18)):
                ko = b.put(kl, residue=r)
                if vl is None:
                    recs.append((ko, kl, U64_MAX, 0))
                else:
                    recs.append((ko, kl, b.put(vl, residue=(5 * r + 3 + kl) % 16), vl))
    c = Case("alignment_grid", b.buf, recs)
    live = c.recs[c.recs[:, 2] != U64_MAX]
    assert len(c.recs) == 5472 and set(c.recs[:, 0] % 16) == set(range(16)) == set(live[:, 2] % 16)
    assert ((live[:, 3] == 0).sum() > 0)                      # empty values beside the deletes
    return c


def _pieces(kl, vl):
    """[(name, start, end)] of a record's pieces, offsets in the record."""
    kp = zf.rup8(kl)
    out = [("key header", 0, 24), ("key", 24, 24 + kl), ("key padding", 24 + kl, 24 + kp)]
    if vl is not None:
        v0 = 24 + kp
        out += [("value header", v0, v0 + 16), ("value", v0 + 16, v0 + 16 + vl),
                ("value padding", v0 + 16 + vl, v0 + 16 + zf.rup8(vl))]
    return out


def tile_boundaries(tile=64):
    """The key length swept 0..80 with a 13-byte value, the value length 0..200
    with a 5-byte key, a 1000-byte value; eight times over, a 24-byte delete
    between the rounds, so that the sweeps meet the tile edges in every phase."""
    lens = []
    for _ in range(8):
        lens += [(kl, 13) for kl in range(81)] + [(5, vl) for vl in range(201)] + [(9, 1000), (0, None)]
    c = from_lengths("tile_boundaries", lens, seed=6)
    # what the list is there for: every kind of piece straddles a tile edge of the file somewhere,
    # a record spans several tiles, one ends exactly on an edge
    at, straddled, ends_on_edge = 40, set(), False
    for kl, vl in lens:
        for name, a, e in _pieces(kl, vl):
            if e - a >= 2 and (at + a) // tile != (at + e - 1) // tile:
                straddled.add(name)
            # padding shares an 8-byte word with the bytes it pads: that word is a tile's last or first
            if name.endswith("padding") and e > a and ((at + a) & ~7) % tile in (0, tile - 8):
                straddled.add(name)
        at += _pieces(kl, vl)[-1][2] if vl is not None else 24 + zf.rup8(kl)
        ends_on_edge |= at % tile == 0
    assert straddled == {"key header", "key", "key padding", "value header", "value", "value padding"}, straddled
    assert ends_on_edge
    return c


def region_sizes():
    """Regions of one 64-byte tile, one tile - 8 and + 8; a file that ends with its first tile."""
    out = []
    for name, lens, region in (("region_64", [(8, 16)], 64), ("region_56", [(8, 8)], 56), ("region_72", [(9, 16)], 72),
                               ("region_24", [(0, None)], 24), ("region_128_two_records", [(8, 16), (3, 11)], 128)):
        c = from_lengths(name, lens, seed=7)
        assert len(c.want) == 40 + region + 8 + 8 * (len(lens) + 1) + 8
        out.append(c)
    return out


def basics():
    return [Case("empty", b"", np.zeros((0, 4), np.uint64)),
            from_pairs("single_kv", [(b"key", b"value-of-the-key")]),
            from_pairs("single_delete", [(b"deleted-key", None)]),
            from_pairs("empty_key_and_value", [(b"", b"")])]


def log_order():
    """The records of records_images.wellformed() in log order (not key order), deletes mixed in."""
    img = ri.wellformed()
    recs, rc = ri.host_records(img, zsfile.ACTIVE)
    assert rc == zsfile.END
    keys = [k for k, _ in ri.as_pairs(img, recs)]
    assert keys != sorted(keys) and 0 < int((recs[:, 2] == U64_MAX).sum()) < len(recs)
    return Case("log_order", img, recs)


def _header_fields(img):
    return img[12:28], int.from_bytes(img[28:32], "big"), int.from_bytes(img[32:36], "big")


def round_trip(name, img):
    """A packed file whose own record list must pack to the same bytes."""
    recs, rc = ri.host_records(img, zsfile.PACKED)
    assert rc == 0
    uuid, s, e = _header_fields(img)
    return Case(name, img, recs, want=img, uuid=uuid, startidx=s, endidx=e)


def round_trips():
    out = [round_trip("packed_small_60", ri.packed_small(60)[0])]
    for rel in ("packed.zs", "repack1/reference_out.zs", "repack2/reference_out.zs", "repack2d/reference_out.zs"):
        with open(os.path.join(GOLDEN, rel), "rb") as fh:
            out.append(round_trip("golden_" + rel.replace("/", "_"), fh.read()))
    return out


def regenerated_headers():
    """packed_long_value_70k: a 70 KB value behind a LONG value header in the
    source; the output has the short header the lengths call for."""
    img, pairs = ri.packed_long_value_70k()
    recs, _ = ri.host_records(img, zsfile.PACKED)
    want = zf.packed_file(pairs, UUID, 1, 9)
    assert want != img and len(want) == len(img)
    return Case("regenerated_headers", img, recs, want=want, startidx=1, endidx=9)


def long_delete():
    c = from_pairs("long_delete", [(b"a", b"1"), (b"D" * 70000, None), (b"z", b"")], seed=8)
    assert zf.be64(0) + zf.be64(70000) + zf.be64(0) + b"DDDD" in c.want
    return c


def shared_bytes():
    """The value pattern of test_pack_batch_api (record i -> the same 40 bytes
    at offset 8 * (i % 5)), keys that overlap each other, the whole list again
    in reverse and every third record a third time."""
    vals = np.arange(80, dtype=np.uint8).tobytes()
    keys = b"".join(b"k%07d" % i for i in range(500))
    src = vals + keys
    recs = []
    for i in range(500):
        # keys of 8..19 bytes that run into the next key's bytes
        recs.append((80 + 8 * i, 8 + i % 12 if i < 498 else 8, U64_MAX if i == 7 else 8 * (i % 5), 40))
    recs = recs + recs[::-1] + recs[::3]
    return Case("shared_bytes", src, recs)


def small_cases():
    """Every list that needs no long form."""
    return basics() + [alignment_grid(), tile_boundaries()] + region_sizes() + [log_order()] + round_trips() + \
        [regenerated_headers(), long_delete(), shared_bytes()]


def records(n, seed, maxval=600, deletes=True):
    """n (key, value or None) pairs in key order, every thirteenth a delete (the host packer's lists)."""
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n):
        key = b"%016d" % (i * 7)
        if deletes and i % 13 == 4:
            recs.append((key, None))
        else:
            recs.append((key, rng.integers(0, 256, int(rng.integers(0, maxval)), dtype=np.uint8).tobytes()))
    return recs


def long_commit_long_records():
    """The list of test_pack_long_commit_long_records (tests/test_gpu_repack.py):
    a 17 MiB value, a 70,000-byte key, an empty value, region above 16 MiB."""
    pairs = records(2500, 9, maxval=9000)
    big = np.random.default_rng(1).integers(0, 256, (17 << 20) + 3, dtype=np.uint8).tobytes()
    pairs.insert(100, (b"%016d" % 700 + b"+big", big))
    pairs.insert(200, (b"%016d" % 1400 + b"+long-key" + b"q" * 70000, b"v" * 33))
    pairs.insert(300, (b"%016d" % 2100 + b"+empty", b""))
    return from_pairs("long_commit_long_records", pairs, seed=9), pairs


def host_packer_file(case, path) -> tuple:
    """(report, bytes) of the host packer (repack.Packer, needs the GPU) for the case's records."""
    src = np.frombuffer(case.src or b"\0", dtype=np.uint8)
    r = case.recs
    with repack.Packer(str(path), case.uuid, case.startidx, case.endidx) as p:
        if len(r):
            p.add_arrays(src, r[:, 0].copy(), r[:, 1].copy(), src, r[:, 2].copy(), r[:, 3].copy())
    with open(path, "rb") as fh:
        return p.report, fh.read()
