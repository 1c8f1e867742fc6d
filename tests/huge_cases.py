"""Small cases moved beyond 4 GiB (tests/test_huge_cases.py on the CPU,
tests/test_gpu_stages_scale.py on the GPU): where a case's blob goes inside an
arena of 2^32 + 768 MiB + 77 bytes so that a key read crosses 2^31 or 2^32,
what the Python models' results become there, and the packed file of a record
list as pieces whose value bodies stay in the arena.  No GPU is needed.

Placements.  Offsets are relative to the source a call is given, so every blob
gets a view of the arena of its own (arena[delta:], deltas 4 MiB apart from 8
MiB on: past the small images behind the huge one, walk_images.huge_image_pieces)
and three places P in that view: byte 3 of a chosen key at offset 2^31
("at_2g"), at 2^32 ("at_4g"), or the blob at 2^32 + 2^29 + 5 ("odd").  A key
of 70,000 bytes has its byte 35,000 there; in a case whose keys are shorter
than four bytes the chosen (longest) key's last byte lies on the boundary.
All blobs lie in the arena at once, at all three places, disjoint.

Expectations.  The models of merge_cases, find_cases, scan_cases and
gather_cases run on the small blob as they always do; shift_*() adds P to the
output words that are offsets and not the delete mark.  A list moves either
base-carried, (recs, base + P), or record-carried, P added into the records."""
import functools

import numpy as np

from oracle import oracle
from oracle import zs_format as zf
from tests import find_cases as fc
from tests import gather_cases as gc
from tests import merge_cases as mc
from tests import scan_cases as sc
from tests.images import U64_MAX
from tests.pack_cases import long_delete_record

B31, B32 = 1 << 31, 1 << 32
ODD_AT = B32 + (1 << 29) + 5
ARENA_BYTES = B32 + (768 << 20) + 77
SLOT0, SLOT = 8 << 20, 4 << 20       # the first view's delta, the distance of two views
PLACES = ("at_2g", "at_4g", "odd")
CARRIES = ("base", "recs")
INLINE_MAX = 4096                    # a value body up to here is a piece of bytes, a longer one stays in the arena


def u64(v) -> np.uint64:
    return np.uint64(v)


# ------------------------------------------------------------------ placements
def straddle_at(key_len: int) -> int:
    """The byte of a key that goes onto the boundary."""
    return 35_000 if key_len >= 70_000 else min(3, key_len - 1)


def chosen_key(recs) -> tuple:
    """(key_off, the byte that goes onto the boundary) of the record list's
    longest key, the last of them (bytes of the blob lie on both sides of the
    boundary then, bytes of the key where it has four)."""
    recs = fc.recs_of(recs)
    i = len(recs) - 1 - int(np.argmax(recs[::-1, 1]))
    assert int(recs[i, 1]) > 0
    return int(recs[i, 0]), straddle_at(int(recs[i, 1]))


class Placed:
    """A blob in its view: delta (the view is arena[delta:]) and the three P."""

    def __init__(self, delta, blob, key_off, at):
        self.delta, self.size, self.key = delta, len(blob), key_off + at
        self.P = {"at_2g": B31 - self.key, "at_4g": B32 - self.key, "odd": ODD_AT}

    def view(self, arena):
        return arena[self.delta:]

    def absolute(self, place) -> int:
        return self.delta + self.P[place]


class Layout:
    """Which bytes go where in the arena; holds the small blobs only."""

    def __init__(self):
        self.writes, self.slots = [], 0

    def place(self, blob: bytes, key_off: int, at: int) -> Placed:
        assert len(blob) < SLOT // 4 and 0 <= key_off + at < len(blob)
        delta = SLOT0 + SLOT * self.slots + (5 * self.slots) % 16        # views at every address residue in turn
        self.slots += 1
        p = Placed(delta, blob, key_off, at)
        for name in PLACES:
            self.writes.append((p.absolute(name), bytes(blob)))
        assert p.absolute("odd") + len(blob) <= ARENA_BYTES
        return p

    def check(self, reserved=()):
        """No two blobs share a byte, none shares one with the (offset, size) spans in `reserved`."""
        spans = sorted([(off, len(b)) for off, b in self.writes] + list(reserved))
        for (a, n), (b, _) in zip(spans[:-1], spans[1:]):
            assert a + n <= b, ("overlap", a, n, b)
        assert spans[-1][0] + spans[-1][1] <= ARENA_BYTES

    def fill(self, put):
        """put(offset, uint8 array) for every blob at every place."""
        for off, b in self.writes:
            if b:
                put(off, np.frombuffer(b, np.uint8))


# ------------------------------------------------------------------ shifts
def shift_recs(recs, P: int) -> np.ndarray:
    """P added to key_off and to every val_off that is not the delete mark."""
    r = fc.recs_of(recs).copy()
    r[:, 0] += u64(P)
    live = r[:, 2] != u64(U64_MAX)
    r[live, 2] += u64(P)
    return r


def shift_hits(hits, P: int) -> np.ndarray:
    """P added to the val_off of the rows that are hits with a value."""
    h = fc.recs_of(hits).copy()
    found = (h[:, 0] < u64(fc.BAD_QUERY)) & (h[:, 2] != u64(U64_MAX))
    h[found, 2] += u64(P)
    return h


def shift_items(items, P: int) -> np.ndarray:
    """P added to the val_off of the gather's items that carry a value."""
    it = gc.items_of(items).copy()
    it[gc.kinds(it)[0], 2] += u64(P)
    return it


def shift_queries(queries, Q: int) -> np.ndarray:
    q = fc.recs_of(queries).copy()
    q[:, 0] += u64(Q)
    return q


def carried(lists, P: int, carry: str) -> list:
    """[(recs, base)] moved by P, by the bases or by the records."""
    assert carry in CARRIES
    if carry == "base":
        return [(fc.recs_of(r), int(b) + P) for r, b in lists]
    return [(shift_recs(r, P), int(b)) for r, b in lists]


def crosses(lists) -> tuple:
    """(a key byte of these lists lies at an offset in [2^31, 2^32), one lies
    at or above 2^32): the tests assert on their inputs that a placement is
    what it says."""
    lo = hi = False
    for r, b in lists:
        r = fc.recs_of(r)
        r = r[r[:, 1] > 0]
        if len(r):
            k = r[:, 0].astype(object) + int(b)
            e = k + r[:, 1].astype(object)
            lo |= bool(((e > B31) & (k < B32)).any())
            hi |= bool((e > B32).any())
    return lo, hi


def expect_crossing(lists, place: str, what=None):
    """at_2g: a key byte in [2^31, 2^32); at_4g: one at or above 2^32; odd:
    every key byte above 2^32 + 2^29."""
    lo, hi = crosses(lists)
    assert {"at_2g": lo and not hi, "at_4g": hi, "odd": hi and not lo}[place], (what, place, lo, hi)
    if place == "odd":
        assert min(int(r[:, 0].min()) + int(b) for r, b in lists if len(r)) > B32 + (1 << 29), what


# ------------------------------------------------------------------ the cases
def merge_list() -> list:
    return [mc.shared_prefix(), mc.key_lengths(), mc.long_keys(), mc.deletes(), mc.random_case(0)]


def find_list() -> list:
    return [fc.one_level(mc.shared_prefix()), fc.one_level(mc.key_lengths()), fc.one_level(mc.long_keys()),
            fc.deletes_case(), fc.random_find_case(0)]


def _scan_of(f: fc.FindCase, step=1) -> sc.ScanCase:
    keys = fc.level_keys(f.src, f.levels[0][0], f.levels[0][1])
    return sc.ScanCase(f.name, f.src, f.levels, *fc.lay_queries(sc.prefixes_of(keys, step)))


def scan_list() -> list:
    return [_scan_of(fc.one_level(mc.shared_prefix()), 3), _scan_of(fc.one_level(mc.key_lengths()), 3),
            _scan_of(fc.one_level(mc.long_keys())), sc.deletes_case(), sc.random_case(0)]


def gather_list() -> list:
    by_name = {c.name: c for c in gc.small_cases()}
    return [by_name[n] for n in ("n257", "lengths64", "front", "ends", "badq_among_good", "tile64_r5")] + \
        [gc.random_case(0, n=400)]


def two_places(case: mc.Case, p: Placed, a: str, b: str, drop: bool):
    """The case's lists in turn at places a and b of its blob, each carrying
    its own base: (lists, winners, result words).  The model runs over the blob
    twice in a row, list j with base 0 or L; an offset below L is then moved
    to a, one from L on to b."""
    L = len(case.src) + (-len(case.src) % 64) + 64
    twice = mc.Case(case.name, case.src + bytes(L - len(case.src)) + case.src,
                    [(r, (j % 2) * L) for j, (r, _) in enumerate(case.lists)])
    w, res = twice.model(drop)
    w = w.copy()
    for col in (0, 2):
        v = w[:, col]
        second = (v >= u64(L)) & (v != u64(U64_MAX))
        first = (v < u64(L))
        v[first] += u64(p.P[a])
        v[second] += u64(p.P[b] - L)
    return [(r, p.P[(a, b)[j % 2]]) for j, (r, _) in enumerate(case.lists)], w, res


class World:
    """Every case with its place in the arena."""

    def __init__(self):
        lay = self.layout = Layout()
        self.merge, self.find, self.scan, self.gather = [], [], [], []
        for c in merge_list():
            recs = np.concatenate([r for r, _ in c.lists])
            self.merge.append((c, lay.place(c.src, *chosen_key(recs))))
        for out, cases in ((self.find, find_list()), (self.scan, scan_list())):
            for c in cases:
                recs = np.concatenate([r for r, _ in c.levels])
                out.append((c, lay.place(c.src, *chosen_key(recs)), lay.place(c.qsrc, *chosen_key(c.queries))))
        for c in gather_list():
            val = c.items[gc.kinds(c.items)[0]]
            i = int(np.argmax(val[:, 3]))
            self.gather.append((c, lay.place(c.src, int(val[i, 2]), straddle_at(int(val[i, 3])))))
        # the packer's list: a small case and one key for the huge record
        from tests import pack_cases as pc
        self.grid = pc.alignment_grid()
        self.grid_at = lay.place(self.grid.src, *chosen_key(self.grid.recs))
        self.huge_key = b"the-key-of-the-huge-record"
        self.huge_key_at = lay.place(self.huge_key, 0, 3)


@functools.lru_cache(maxsize=1)
def world() -> World:
    return World()


# ------------------------------------------------------- the packed file as pieces
_BIG = 1 << 20
_big_crcs = {}


def span_crc(host: np.ndarray, off: int, n: int) -> int:
    """crc32c(0, host[off:off + n]) by the oracle, a long span in 64 MiB parts on
    eight threads folded by the oracle's combine; kept for the next caller."""
    key = (host.ctypes.data, off, n)
    if key not in _big_crcs:
        part = 64 << 20
        offs = np.arange(off, off + n, part, dtype=np.uint64)
        lens = np.minimum(u64(off + n) - offs, u64(part))
        crcs = oracle.batch(host, offs, lens, impl="hw", threads=8)
        c = int(crcs[0])
        for pc_, ln in zip(crcs[1:].tolist(), lens[1:].tolist()):
            c = oracle.combine(c, pc_, ln)
        _big_crcs[key] = c
    return _big_crcs[key]


def _value_header(n: int) -> bytes:
    """The 16 bytes in front of a value of n bytes (zf.value_record's head)."""
    if n > zf.MAX_SHORT_VAL_LEN:
        return zf.be64(zf.REC_LONG_VALUE << 56) + zf.be64(n)
    return zf.be64((zf.REC_VALUE << 56) | (n << 32)) + zf.be64(0)


class Packed:
    """runs [(file_off, bytes)], bodies [(file_off, arena_off, length)],
    file_bytes, recs (the file's own record list, file coordinates) and the
    eight result words of zscrc_device_pack."""

    def assembled(self, host) -> bytes:
        out = bytearray(self.file_bytes)
        for at, b in self.runs:
            out[at:at + len(b)] = b
        for at, src, n in self.bodies:
            out[at:at + n] = host[src:src + n].tobytes()
        return bytes(out)


def packed_pieces(host: np.ndarray, recs, uuid: bytes, startidx: int, endidx: int) -> Packed:
    """The packed file of the records `recs` (absolute offsets into host, a
    uint8 array) in the order given."""
    recs = fc.recs_of(recs)
    p = Packed()
    p.runs, p.bodies = [], []
    run, run_at = bytearray(zf.header_bytes(uuid, startidx, endidx)), 0
    hashed = len(run)                   # bytes of `run` the span's CRC has taken in (the header: none of it counts)
    at, crc = len(run), 0
    ptrs, frecs = [], []

    def take():
        nonlocal crc, hashed
        if hashed < len(run):
            crc = oracle.crc32c_hw(crc, np.frombuffer(run, np.uint8)[hashed:])
            hashed = len(run)

    def close():
        nonlocal run, run_at, hashed
        take()
        if run:
            p.runs.append((run_at, bytes(run)))
        run, run_at, hashed = bytearray(), at, 0

    for ko, kl, vo, vl in recs.tolist():
        ptrs.append(at)
        key = host[ko:ko + kl].tobytes()
        if vo == U64_MAX:
            rec = long_delete_record(key) if kl > zf.MAX_SHORT_KEY_LEN else zf.delete_record(key)
            frecs.append((at + 24, kl, U64_MAX, 0))
            run += rec
            at += len(rec)
            continue
        rec = zf.key_record(key) + _value_header(vl)
        run += rec
        at += len(rec)
        frecs.append((at - len(rec) + 24, kl, at, vl))
        if vl <= INLINE_MAX:
            run += host[vo:vo + vl].tobytes()
        else:
            close()
            p.bodies.append((at, vo, vl))
            if vl >= _BIG:
                crc = oracle.combine(crc, span_crc(host, vo, vl), vl)
            else:
                crc = oracle.crc32c_hw(crc, host[vo:vo + vl])
            run_at = at + vl
        at += vl
        run += bytes(zf.rup8(vl) - vl)
        at += zf.rup8(vl) - vl
    take()
    region = at - zf.HDR_SIZE
    commit = zf.commit_record(crc, region)
    run += commit
    at += len(commit)
    hashed = len(run)
    ptr = zf.be64(len(ptrs)) + b"".join(zf.be64(q) for q in ptrs)
    pcrc = oracle.crc32c_hw(0, ptr)
    final = zf.commit_record(pcrc, len(ptr), final=True)
    run += ptr + final
    at += len(ptr) + len(final)
    p.runs.append((run_at, bytes(run)))
    p.file_bytes = at
    p.recs = fc.recs_of(frecs)
    p.res = [0, len(recs), at, region, crc, pcrc, int.from_bytes(commit[-4:], "big"), int.from_bytes(final[-4:], "big")]
    p.pointers_at = at - len(final) - len(ptr)
    return p


# ------------------------------------------------------- a merge model over the arena
def merge_model(host: np.ndarray, lists, drop_deletes: bool):
    """mc.Case.model for lists whose records lie anywhere in `host`: the keys
    are copied into a small blob (one byte between them, so that every record
    keeps an offset of its own), the model runs over that, and its winners are
    taken back to the records they came from."""
    recs = mc.Case("arena", b"", lists).rebased()
    blob, small, back = bytearray(), recs.copy(), {}
    for i, (ko, kl) in enumerate(recs[:, :2].tolist()):
        small[i, 0] = len(blob)
        back[len(blob)] = ko
        blob += host[ko:ko + kl].tobytes() + b"\xEE"
    w, res = mc.Case("arena", blob, [(small, 0)]).model(drop_deletes)
    w = w.copy()
    w[:, 0] = [back[int(o)] for o in w[:, 0]]
    return w, res
