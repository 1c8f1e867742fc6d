"""The model and the cases of the value gather's tests (tests/test_gather_host.py
and tests/test_gather_layout.py on the CPU, tests/test_gpu_gather.py on the
GPU).  The model is pure Python and numpy: slices of the source laid end to
end, oracle.crc32c_hw(0, value) for the CRCs and the eight result words of
include/zscrc.h.  No GPU is needed."""
import struct

import numpy as np

from oracle import oracle
from tests.images import EINVAL64, OVERFLOW, U64_MAX  # noqa: F401  (the tests read them as gc.*)

NONE, BAD_QUERY, DELETED = U64_MAX, U64_MAX - 1, U64_MAX
FILL = 0x3333333333333333  # word 1 of an item: never read


def items_of(rows) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(rows, dtype=np.uint64).reshape(-1, 4))


def value(off, ln):
    return (0, FILL, off, ln)


MISS = (NONE, 7, 0, 0)               # a lower bound in word 1, as the find leaves it
BADQ = (BAD_QUERY, 0, 0, 0)
DELETE = (0, FILL, DELETED, 0)
# a miss and a bad query whose value words would be far outside any source if they were read
WILD_MISS = (NONE, 0, 1 << 61, 1 << 63)
WILD_BADQ = (BAD_QUERY, 0, U64_MAX - 1, U64_MAX)


def kinds(items: np.ndarray):
    """(has a value, delete, not found, bad query) as boolean arrays."""
    badq = items[:, 0] == np.uint64(BAD_QUERY)
    none = items[:, 0] == np.uint64(NONE)
    dele = ~badq & ~none & (items[:, 2] == np.uint64(DELETED))
    return ~badq & ~none & ~dele, dele, none, badq


def model(src: bytes, items, cap=None, crcs=True):
    """(values uint8 array or None, offs uint64 [nq + 1] or None, crcs uint32
    [nq] or None, the eight result words).  cap=None: room for every value.
    values is None where nothing of the output is written (a code other than
    0), offs where nothing of the offsets is (EINVAL)."""
    items = items_of(items)
    nq, size = len(items), len(src)
    val, dele, none, badq = kinds(items)
    vo, vl = items[:, 2], items[:, 3]
    left = np.uint64(size) - np.minimum(vo, np.uint64(size))
    bad = val & ((vo > np.uint64(size)) | (vl > left))
    zero = np.zeros(nq, np.uint32) if crcs else None
    if bad.any():
        return None, None, zero, [EINVAL64, int(np.flatnonzero(bad)[0]), 0, 0, 0, 0, 0, 0]
    lens = np.where(val, vl, np.uint64(0))
    offs = np.zeros(nq + 1, np.uint64)
    np.cumsum(lens, out=offs[1:])
    total = int(offs[nq])
    res = [0, nq, int(val.sum()), total, int(dele.sum()), int(none.sum()), int(badq.sum()),
           int(lens.max()) if nq else 0]
    if cap is not None and total > cap:
        res[0] = OVERFLOW
        return None, offs, zero, res
    s = np.frombuffer(src, np.uint8)
    idx = np.repeat((vo - offs[:-1])[val], lens[val].astype(np.int64)) + np.arange(total, dtype=np.uint64)
    values = s[idx.astype(np.int64)] if total else np.zeros(0, np.uint8)
    out = None
    if crcs:
        vb = values.tobytes()
        o = offs.tolist()
        out = np.array([oracle.crc32c_hw(0, vb[o[i]:o[i + 1]]) if o[i + 1] > o[i] else 0 for i in range(nq)],
                       np.uint32).reshape(nq)
    return values, offs, out, res


def slices(src: bytes, items) -> list:
    """The model's values one by one, the plain way: None for an item without one."""
    items = items_of(items)
    return [bytes(src[o:o + n]) if v else None for v, (_, _, o, n) in zip(kinds(items)[0], items.tolist())]


class GatherCase:
    def __init__(self, name, src, items):
        self.name, self.src, self.items = name, bytes(src), items_of(items)

    def model(self, cap=None, crcs=True):
        return model(self.src, self.items, cap, crcs)

    @property
    def nq(self):
        return len(self.items)

    def case_file(self, shift=0, want=None) -> bytes:
        """The case as tests/c/gather_layout.cpp reads it."""
        values, offs, _, res = self.model(crcs=False)
        want = values.tobytes() if want is None else want
        head = struct.pack("<4Q", len(self.src), self.nq, shift, len(want))
        return head + self.src + self.items.tobytes() + want


def source(n: int, seed=0) -> bytes:
    return np.random.default_rng(1000 + seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def lengths_case(name, lengths, seed=0) -> GatherCase:
    """Values of these lengths (None: a miss, a delete or a bad query in
    turn), value i from a source offset = i mod 16 past a multiple of 16."""
    big = max([n for n in lengths if n] or [0])
    src = source(big + 16 * 64 + 64, seed)
    rows, k = [], 0
    for i, n in enumerate(lengths):
        if n is None:
            rows.append((MISS, DELETE, BADQ, WILD_MISS, WILD_BADQ)[k % 5])
            k += 1
        else:
            rows.append(value(16 * ((7 * i) % 64) + i % 16, n))
    return GatherCase(name, src, rows)


def mixed_lengths(n: int, seed: int, hi=40, none=3) -> list:
    """n lengths from 0 to hi, about one in `none` of them None."""
    rng = np.random.default_rng(seed)
    ln = rng.integers(0, hi + 1, n).tolist()
    drop = rng.integers(0, none, n) == 0
    return [None if d else v for v, d in zip(ln, drop.tolist())]


def counted_case(n: int) -> GatherCase:
    return lengths_case("n%d" % n, mixed_lengths(n, n))


COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097)


def tile_lengths(tile: int) -> list:
    return [0, 1, 7, 8, 9, 15, 16, 17, 31, 33, tile - 1, tile, tile + 1, 3 * tile + 5]


def residue_case(tile: int, r: int) -> GatherCase:
    """tile_lengths(tile), every value from a source offset = r mod 16, behind
    r one-byte values so that the outputs shift too."""
    lens = tile_lengths(tile)
    src = source(3 * tile + 5 + 64, tile + r)
    return GatherCase("tile%d_r%d" % (tile, r), src,
                      [value(40 + i, 1) for i in range(r)] + [value(16 + r, n) for n in lens])


def front_case() -> GatherCase:
    """Lengths 0 .. 15 in front: the values after them start at every output residue mod 16."""
    return lengths_case("front", [k for n in range(16) for k in (n, 33, (-n - 33) % 16)] + [100])


def ends_case() -> GatherCase:
    """A value at source byte 0, one that ends with the source's last byte, the whole source, empty ones at both ends."""
    src = source(777, 5)
    return GatherCase("ends", src, [value(0, 0), value(0, 13), value(777 - 29, 29), value(777, 0), value(0, 777),
                                     value(776, 1), value(777, 0)])


def no_values_case(kind) -> GatherCase:
    return GatherCase("only_%s" % {MISS: "misses", DELETE: "deletes", BADQ: "badq"}[kind], source(64), [kind] * 300)


def badq_case() -> GatherCase:
    rows = [value(3 * i, i % 19) for i in range(200)]
    for i in (0, 5, 77, 199):
        rows[i] = WILD_BADQ
    return GatherCase("badq_among_good", source(700, 9), rows)


def misses_between_case() -> GatherCase:
    """10,000 misses between two values, at the front and at the end of the list."""
    gap = [MISS] * 10_000
    return GatherCase("misses_between", source(300, 11),
                      gap + [value(5, 50)] + gap + [value(100, 37), value(1, 1)] + [WILD_MISS] * 10_000)


def one_byte_case(n=2 * 65536 + 11) -> GatherCase:
    """More one-byte values than any stage of starts holds."""
    src = source(4099, 13)
    items = np.zeros((n, 4), np.uint64)
    items[:, 1] = FILL
    items[:, 2] = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(4099)
    items[:, 3] = 1
    return GatherCase("one_byte", src, items)


def long_value_case() -> GatherCase:
    """One value of 3 MiB + 5 among short ones, and one source value under two items."""
    big = 3 * (1 << 20) + 5
    src = source(big + 100, 17)
    return GatherCase("long_value", src, [value(1, 9), value(50, 20), value(3, big), value(50, 20), MISS, value(7, 3)])


def million_case() -> GatherCase:
    """2^20 + 1 items of 0 to 3 bytes: more than 1,024 block sums for the one-workgroup scan."""
    n = (1 << 20) + 1
    rng = np.random.default_rng(23)
    src = source(8191, 19)
    items = np.zeros((n, 4), np.uint64)
    items[:, 1] = FILL
    items[:, 2] = rng.integers(0, 8188, n).astype(np.uint64)
    items[:, 3] = rng.integers(0, 4, n).astype(np.uint64)
    return GatherCase("million", src, items)


def random_case(seed: int, n=2000) -> GatherCase:
    """n items, lengths from 0 to 5,000 (half of them short), about a third without a value."""
    rng = np.random.default_rng(5000 + seed)
    src = source(20_000 + seed, seed)
    size = len(src)
    rows = []
    for i in range(n):
        k = int(rng.integers(0, 9))
        if k < 3:
            rows.append((MISS, DELETE, WILD_BADQ)[k])
            continue
        ln = int(rng.integers(0, 5001)) if k < 6 else int(rng.integers(0, 40))
        rows.append(value(int(rng.integers(0, size - ln + 1)), ln))
    return GatherCase("random%d" % seed, src, rows)


def small_cases() -> list:
    """The cases every implementation is held against (the GPU adds the large ones)."""
    out = [counted_case(n) for n in COUNTS]
    out += [lengths_case("lengths64", [n for n in tile_lengths(64) for _ in range(3)], 3), front_case(), ends_case(),
            no_values_case(MISS), no_values_case(DELETE), no_values_case(BADQ), badq_case(), misses_between_case()]
    out += [residue_case(64, r) for r in range(16)]
    return out
