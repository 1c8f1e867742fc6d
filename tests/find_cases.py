"""The model and the cases of the lookup's tests (tests/test_find_host.py and
tests/test_find_order.py on the CPU, tests/test_gpu_find.py on the GPU).  The
model is Python's bisect_left over the levels' key bytes -- the order of
Python's bytes is memcmp_raw.  Levels come from tests/merge_cases.py unchanged:
case.model(False)[0] is a strictly ascending list over case.src.  No GPU is
needed."""
import struct
from bisect import bisect_left

import numpy as np

from tests import merge_cases as mc
from tests.images import EINVAL64, U64_MAX  # noqa: F401  (the tests read them as fc.*)

NONE, BAD_QUERY = U64_MAX, U64_MAX - 1


def recs_of(r) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(r, dtype=np.uint64).reshape(-1, 4))


def level_keys(src: bytes, recs, base: int) -> list:
    return [src[int(o) + base:int(o) + base + int(ln)] for o, ln in recs_of(recs)[:, :2]]


def model(src: bytes, levels, qsrc: bytes, queries):
    """(hits uint64 [nq, 4], the eight result words) for levels = [(recs, base)]
    whose records lie inside src and ascend."""
    src, qsrc = bytes(src), bytes(qsrc)
    levels = [(recs_of(r), int(b)) for r, b in levels]
    keys = [level_keys(src, r, b) for r, b in levels]
    queries = recs_of(queries)
    hits = np.zeros((len(queries), 4), np.uint64)
    res = [0, len(queries), 0, 0, 0, 0, 0, 0]
    for i, (off, ln) in enumerate(queries[:, :2].tolist()):
        if off > len(qsrc) or ln > len(qsrc) - off:
            hits[i, 0] = BAD_QUERY
            res[5] += 1
            continue
        q = qsrc[off:off + ln]
        hits[i] = (NONE, bisect_left(keys[-1], q) if keys else 0, 0, 0)
        for l, (recs, base) in enumerate(levels):
            at = bisect_left(keys[l], q)
            if at < len(recs) and keys[l][at] == q:
                vo = int(recs[at, 2])
                hits[i] = (l, at, vo if vo == U64_MAX else vo + base, int(recs[at, 3]))
                break
        if int(hits[i, 0]) == NONE:
            res[4] += 1
        elif int(hits[i, 2]) == U64_MAX:
            res[3] += 1
        else:
            res[2] += 1
            res[6] = (res[6] + int(hits[i, 3])) & U64_MAX
    return hits, res


def lay_queries(keys, residue=None, pad_end=True):
    """(blob, queries [nq, 4]): the keys one after another, each at offset =
    residue mod 8 if given; the value words hold a pattern no search may read
    anything from."""
    buf, q = bytearray(), []
    for k in keys:
        if residue is not None:
            buf += b"\xDD" * ((residue - len(buf)) % 8)
        q.append((len(buf), len(k), 0x7777777777777777, 0x5555555555555555))
        buf += k
    if pad_end:
        buf += b"\xDD" * 3
    return bytes(buf), recs_of(q)


def probe_keys(keys) -> list:
    """Every key, every key with a byte appended, one key below the first and
    one above the last, the empty key."""
    keys = list(keys)
    out = keys + [k + b"\x00" for k in keys] + [k + b"\xff" for k in keys[::3]] + [b""]
    if keys:
        lo, hi = min(keys), max(keys)
        out += [lo[:-1] if lo else b"", hi + b"\xff\xff"]
        if lo and lo[-1]:
            out.append(lo[:-1] + bytes([lo[-1] - 1]))
    return out


def sorted_level(case: mc.Case):
    """The case's winners: one strictly ascending level over case.src, base 0."""
    return case.model(False)[0]


def counted_level(n: int, seed=1):
    """(src, recs): a level of exactly n records, `key-` + 8 digits ascending, every eleventh a delete."""
    rng = np.random.default_rng(seed + n)
    ids = np.sort(rng.choice(max(3 * n, 1), n, replace=False)) if n else []
    c = mc.from_items("level%d" % n, [(b"key-%08d" % int(k), None if i % 11 == 5 else b"v%d" % i)
                                     for i, k in enumerate(ids)])
    recs = c.lists[0][0] if c.lists else recs_of([])
    assert len(recs) == n
    return c.src, recs


class FindCase:
    """src, levels [(recs, base)], the query blob and the queries."""

    def __init__(self, name, src, levels, qsrc, queries):
        self.name, self.src, self.qsrc = name, bytes(src), bytes(qsrc)
        self.levels = [(recs_of(r), int(b)) for r, b in levels]
        self.queries = recs_of(queries)

    def model(self):
        return model(self.src, self.levels, self.qsrc, self.queries)

    @property
    def n(self):
        return sum(len(r) for r, _ in self.levels)

    def case_file(self, shift=0, qshift=0, want=None) -> bytes:
        """The case as tests/c/find_order.cpp reads it."""
        want = self.model()[0] if want is None else want
        recs = np.concatenate([r for r, _ in self.levels]) if self.levels else recs_of([])
        head = struct.pack("<7Q", len(self.src), len(self.levels), len(recs), len(self.qsrc), len(self.queries),
                           shift, qshift)
        return head + b"".join(struct.pack("<2Q", len(r), b) for r, b in self.levels) + self.src + recs.tobytes() + \
            self.qsrc + self.queries.tobytes() + np.ascontiguousarray(want, np.uint64).tobytes()


def one_level(case: mc.Case, residue=None) -> FindCase:
    recs = sorted_level(case)
    qsrc, queries = lay_queries(probe_keys(level_keys(case.src, recs, 0)), residue)
    return FindCase(case.name, case.src, [(recs, 0)], qsrc, queries)


def counted_case(n: int, residue=None) -> FindCase:
    src, recs = counted_level(n)
    qsrc, queries = lay_queries(probe_keys(level_keys(src, recs, 0)), residue)
    return FindCase("n%d" % n, src, [(recs, 0)], qsrc, queries)


def split_levels(case: mc.Case):
    """Each list of the case as a level of its own: that list's winners."""
    return [(sorted_level(mc.Case(case.name, case.src, [(r, b)])), 0) for r, b in case.lists]


def deletes_case() -> FindCase:
    """Three levels with an empty one between: a is a delete in level 0 and a
    value in level 2, b the reverse, c only in the last level, d in none."""
    c = mc.from_items("lv", [(b"a", None), (b"b", b"new"), (b"m", b"0"), (b"a", b"old"), (b"b", None), (b"c", b"last"),
                             (b"x", b"2")], cuts=(3,))
    l0, l2 = split_levels(c)
    qsrc, queries = lay_queries([b"a", b"b", b"c", b"d", b"m", b"x", b"", b"zz"])
    return FindCase("deletes", c.src, [l0, (recs_of([]), 99), l2], qsrc, queries)


def twice_case() -> FindCase:
    """One list under two bases: level 0 wins every key."""
    c = mc.twice()
    one = sorted_level(mc.Case("once", c.src, [c.lists[0]]))
    qsrc, queries = lay_queries(probe_keys(level_keys(c.src, one, 0)))
    return FindCase("twice", c.src, [(one, 0), (one, c.lists[1][1])], qsrc, queries)


def random_find_case(seed: int, nq=3000) -> FindCase:
    """mc.random_case(seed) as 1 to 4 levels, each its own list's winners, and
    nq queries from the same key generator."""
    c = mc.random_case(seed)
    rng = np.random.default_rng(7000 + seed)
    keys = [rng.integers(97, 100, int(rng.integers(0, 21)), dtype=np.uint8).tobytes() for _ in range(nq)]
    qsrc, queries = lay_queries(keys, residue=seed % 8 if seed % 3 else None)
    return FindCase("random%d" % seed, c.src, split_levels(c), qsrc, queries)


def small_cases() -> list:
    """The cases every implementation is held against."""
    by_name = {c.name: c for c in mc.small_cases()}
    out = [FindCase("no_levels", b"", [], *lay_queries([b"", b"k"])),
           FindCase("empty_levels", b"abc", [(recs_of([]), 0)] * 3, *lay_queries([b"", b"k", b"abc"]))]
    out += [counted_case(n) for n in (0, 1, 2, 3, 4, 5, 8, 63, 64, 65, 129, 194)]
    out += [one_level(by_name[n]) for n in ("shared_prefix", "key_lengths", "ends_at_last_byte", "long_keys")]
    out += [one_level(by_name["residue%d" % r], residue=(r + 3) % 8) for r in range(8)]
    out += [deletes_case(), twice_case()]
    return out
