"""The model and the cases of the prefix scan's tests (tests/test_scan_host.py
and tests/test_scan_order.py on the CPU, tests/test_gpu_scan.py on the GPU).
The model is a dictionary filled from the oldest level to the newest over each
level's matching keys, then sorted, deletes dropped or kept -- the order of
Python's bytes is memcmp_raw and startswith is the match.  Levels come from
tests/merge_cases.py and tests/find_cases.py.  No GPU is needed."""
import struct

import numpy as np

from tests import find_cases as fc
from tests import merge_cases as mc

U64_MAX = fc.U64_MAX
EINVAL64 = fc.EINVAL64
OVERFLOW = mc.OVERFLOW
RES_WORDS = 12
recs_of = fc.recs_of
NO_COMPARE = "no expected rows"


def model(src: bytes, levels, qsrc: bytes, queries, keep_deletes: bool):
    """(rows uint64 [m, 4], offs [nq + 1], seqs [m], the twelve result words)
    for levels = [(recs, base)] whose records lie inside src and ascend."""
    src, qsrc = bytes(src), bytes(qsrc)
    levels = [(recs_of(r), int(b)) for r, b in levels]
    keys = [fc.level_keys(src, r, b) for r, b in levels]
    firsts = np.cumsum([0] + [len(r) for r, _ in levels])
    queries = recs_of(queries)
    rows, seqs, offs = [], [], [0]
    res = [0, len(queries)] + [0] * (RES_WORDS - 2)
    seen = {}
    for off, ln in queries[:, :2].tolist():
        if off > len(qsrc) or ln > len(qsrc) - off:
            res[6] += 1
            offs.append(len(rows))
            continue
        p = qsrc[off:off + ln]
        if p not in seen:       # (candidates, [(row, seq)] of the winners in key order)
            cand, newest = 0, {}
            for l in reversed(range(len(levels))):
                for j, key in enumerate(keys[l]):
                    if key.startswith(p):
                        cand += 1
                        newest[key] = (l, j)
            won = []
            for key in sorted(newest):
                l, j = newest[key]
                recs, base = levels[l]
                ko, kl, vo, vl = (int(v) for v in recs[j])
                won.append(((ko + base, kl, vo if vo == U64_MAX else vo + base, vl), int(firsts[l]) + j))
            seen[p] = (cand, won)
        cand, won = seen[p]
        res[3] += cand
        res[4] += cand - len(won)
        for row, seq in won:
            dele = row[2] == U64_MAX
            res[5] += dele
            if dele and not keep_deletes:
                continue
            rows.append(row)
            seqs.append(seq)
            res[8] += row[1]
            res[9] += 0 if dele else row[3]
        offs.append(len(rows))
    res[2] = len(rows)
    return recs_of(rows), np.asarray(offs, np.uint64), np.asarray(seqs, np.uint64), res


class ScanCase:
    """src, levels [(recs, base)], the prefix blob and the prefixes as queries."""

    def __init__(self, name, src, levels, qsrc, queries):
        self.name, self.src, self.qsrc = name, bytes(src), bytes(qsrc)
        self.levels = [(recs_of(r), int(b)) for r, b in levels]
        self.queries = recs_of(queries)
        self._model = {}

    def model(self, keep_deletes: bool):
        """Computed once a flag and shared: treat the arrays as read-only."""
        if keep_deletes not in self._model:
            self._model[keep_deletes] = model(self.src, self.levels, self.qsrc, self.queries, keep_deletes)
        return self._model[keep_deletes]

    @property
    def n(self):
        return sum(len(r) for r, _ in self.levels)

    def case_file(self, keep_deletes: bool, shift=0, qshift=0, want=None) -> bytes:
        """The case as tests/c/scan_order.cpp reads it; want = NO_COMPARE: no
        expected rows, the program only runs and checks its positions."""
        recs = np.concatenate([r for r, _ in self.levels]) if self.levels else recs_of([])
        body = b"".join(struct.pack("<2Q", len(r), b) for r, b in self.levels) + self.src + recs.tobytes() + \
            self.qsrc + self.queries.tobytes()
        m = U64_MAX
        if want is not NO_COMPARE:
            rows, offs, seqs, _ = self.model(keep_deletes) if want is None else want
            m = len(rows)
            body += np.ascontiguousarray(offs, np.uint64).tobytes() + np.ascontiguousarray(rows, np.uint64).tobytes() + \
                np.ascontiguousarray(seqs, np.uint64).tobytes()
        return struct.pack("<9Q", len(self.src), len(self.levels), len(recs), len(self.qsrc), len(self.queries), shift,
                           qshift, int(keep_deletes), m) + body


def prefixes_of(keys, step=1) -> list:
    """The empty prefix, and of every step-th key its first one, two and half
    of its bytes, the key, the key with a byte appended and the key with its
    last byte raised by one."""
    out = [b""]
    for k in list(keys)[::step]:
        out += [k[:1], k[:2], k[:len(k) // 2], k, k + b"\x00"]
        if k and k[-1] < 255:
            out.append(k[:-1] + bytes([k[-1] + 1]))
    return out


def from_items(name, items, prefixes, cuts=(), residue=None, qresidue=None) -> ScanCase:
    """items in input order cut into lists (mc.from_items), each list's winners a level."""
    c = mc.from_items(name, items, cuts=cuts, residue=residue)
    return ScanCase(name, c.src, fc.split_levels(c), *fc.lay_queries(prefixes, qresidue))


def counted_case(n: int) -> ScanCase:
    src, recs = fc.counted_level(n)
    keys = fc.level_keys(src, recs, 0)
    pre = prefixes_of(keys, max(1, n // 7)) + [b"key-", b"key-0000", b"key-00000", b"kez", b"a"]
    return ScanCase("n%d" % n, src, [(recs, 0)], *fc.lay_queries(pre))


def many_levels_case() -> ScanCase:
    """64 levels: 40 of a few records each, the keys shared between them, 24 empty ones between."""
    rng = np.random.default_rng(64)
    items, cuts = [], []
    for l in range(40):
        for key in sorted(set(int(v) for v in rng.integers(0, 60, int(rng.integers(1, 6))))):
            items.append((b"k%02d" % key, None if rng.integers(0, 4) == 0 else b"v%d.%d" % (l, key)))
        cuts.append(len(items))
    c = mc.from_items("many_levels", items, cuts=cuts[:-1])
    full, levels = fc.split_levels(c), []
    for l, lv in enumerate(full):
        levels.append(lv)
        if l % 5 < 3:
            levels.append((recs_of([]), 7 * l))
    assert len(levels) == 64
    return ScanCase("many_levels", c.src, levels, *fc.lay_queries([b"", b"k", b"k0", b"k1", b"k5", b"k33", b"k6", b"l"]))


PREFIX_KEYS = [b"ab", b"ab\x00", b"ab\x00\x00", b"abc", b"abcd", b"abd", b"a", b"a\xff", b"a\xff\xff", b"b", b"ba",
               b"c\xff\xfe", b"c\xff\xff\x01"]


def prefix_case(prefixes, name="prefixes") -> ScanCase:
    """One level of PREFIX_KEYS over an older level of some of them."""
    items = [(k, b"new-" + k) for k in PREFIX_KEYS] + [(k, b"old-" + k) for k in PREFIX_KEYS[::2]] + [(b"bb", b"only")]
    return from_items(name, items, prefixes, cuts=(len(PREFIX_KEYS),))


PREFIXES = [b"", b"ab", b"ab\x00", b"abc", b"a\xff", b"a\xff\xff", b"\xff", b"c\xff", b"c\xff\xff", b"A", b"aa", b"zz",
            b"abcdefghijklmnopqrstuvwxyz-longer-than-every-key", b"a", b"ab", b"abc", b"b", b"ab\x00\x00", b"ab\x00\x00\x00"]


def long_prefix_case() -> ScanCase:
    """Prefixes of 7, 8, 9, 15, 16, 17 and 70,000 bytes over keys that share them and differ just after."""
    stem = np.random.default_rng(6).integers(1, 255, 70001, dtype=np.uint8).tobytes()
    lens = (7, 8, 9, 15, 16, 17, 70000)
    keys = sorted({stem[:ln] + t for ln in lens for t in (b"", b"\x00", b"\xff", stem[ln:ln + 1])})
    items = [(k, b"v%d" % i) for i, k in enumerate(keys)]
    pre = [stem[:ln] for ln in lens] + [stem[:ln - 1] + bytes([stem[ln - 1] + 1]) for ln in lens] + [stem, stem + b"x"]
    return from_items("long_prefixes", items[::2] + items[1::2] + items[::3], pre, cuts=(len(items[::2]),))


def winners_case() -> ScanCase:
    """Three levels: a newer delete over an older value and the reverse, a key
    in every level, a key only in the last one."""
    items = [(b"k.del-over-value", None), (b"k.every", b"0"), (b"k.value-over-del", b"new"), (b"k.zero", b"z"),
             (b"k.every", b"1"), (b"k.mid", None),
             (b"k.del-over-value", b"old"), (b"k.every", None), (b"k.last", b"last"), (b"k.value-over-del", None)]
    return from_items("winners", items, [b"", b"k.", b"k.e", b"k.del", b"k.l", b"k.value-over-del", b"j", b"l"],
                      cuts=(4, 6))


def candidates_case(c: int) -> ScanCase:
    """Exactly c candidates in one level of 4,096 records: `a` and 4,095 keys
    with k, under empty prefixes (4,096 each), then k (4,095) or a (1)."""
    items = [(b"a", b"first")] + [(b"k%05d" % i, None if i % 13 == 5 else b"%d" % i) for i in range(4095)]
    pre = [b""] * (c // 4096)
    rest = c % 4096
    if rest == 4095:
        pre.append(b"k")
    elif rest:
        assert rest == 1
        pre.append(b"a")
    case = from_items("c%d" % c, items, pre)
    return case


def one_level_count_case(n: int) -> ScanCase:
    """The empty prefix over one level of n records: n candidates."""
    src, recs = fc.counted_level(n)
    return ScanCase("c%d" % n, src, [(recs, 0)], *fc.lay_queries([b""]))


def nq_case(nq: int) -> ScanCase:
    pre = (PREFIXES * (nq // len(PREFIXES) + 1))[:nq]
    return prefix_case(pre, "nq%d" % nq)


def bad_queries_case() -> ScanCase:
    c = prefix_case([b"", b"ab", b"zz", b"a", b"b", b"abc"], "bad_queries")
    q = c.queries.copy()
    q[1] = (len(c.qsrc) + 1, 0, 0, 0)            # starts past the end
    q[2] = (len(c.qsrc) - 1, 2, 0, 0)            # ends one byte past it
    q[4] = (U64_MAX, 1, 0, 0)
    return ScanCase("bad_queries", c.src, c.levels, c.qsrc, q)


def residue_case(r: int) -> ScanCase:
    c = mc.residues(r)
    recs = fc.sorted_level(c)
    keys = fc.level_keys(c.src, recs, 0)
    older = recs[::3].copy()
    pre = prefixes_of(keys, 5) + [b"a", b"b", b"c", b"ab", b"abc", b"cc"]
    return ScanCase("residue%d" % r, c.src, [(recs[1::2], 0), (older, 0)], *fc.lay_queries(pre, (r + 3) % 8))


def random_case(seed: int, nq=100) -> ScanCase:
    """fc.random_find_case(seed)'s levels under prefixes of 0 to 3 letters."""
    f = fc.random_find_case(seed, nq=1)
    rng = np.random.default_rng(9000 + seed)
    pre = [rng.integers(97, 100, int(rng.integers(0, 4)), dtype=np.uint8).tobytes() for _ in range(nq)]
    return ScanCase("random%d" % seed, f.src, f.levels, *fc.lay_queries(pre, seed % 8 if seed % 3 else None))


def twice_case() -> ScanCase:
    f = fc.twice_case()
    keys = fc.level_keys(f.src, f.levels[0][0], 0)
    return ScanCase("twice", f.src, f.levels, *fc.lay_queries(prefixes_of(keys, 40)))


def deletes_case() -> ScanCase:
    f = fc.deletes_case()
    return ScanCase("deletes", f.src, f.levels, *fc.lay_queries([b"", b"a", b"b", b"c", b"d", b"m", b"x", b"zz"]))


# C one below, at and one above the workgroup (256), the block of the scans
# (1,024) and the rank's persistent grid (zsfile.SCAN_GRID_THREADS, 262,144)
GRID_THREADS = 262144
WG, BLOCK = 256, 1024          # zscrc_internal.h WG; zsfile.SCAN_BLOCK (the tests assert it)
SMALL_COUNTS = (1, WG - 1, WG, WG + 1, BLOCK - 1, BLOCK, BLOCK + 1)
GRID_COUNTS = (GRID_THREADS - 1, GRID_THREADS, GRID_THREADS + 1)


def small_cases() -> list:
    """The cases every implementation is held against."""
    out = [ScanCase("no_levels", b"", [], *fc.lay_queries([b"", b"k"])),
           ScanCase("empty_levels", b"abc", [(recs_of([]), 0)] * 3, *fc.lay_queries([b"", b"k", b"abc"])),
           ScanCase("no_match", counted_case(5).src, counted_case(5).levels, *fc.lay_queries([b"nothing"]))]
    out += [counted_case(n) for n in (0, 1, 2, 3, 63, 64, 65)]
    out += [many_levels_case(), twice_case(), deletes_case(), winners_case()]
    out += [prefix_case(PREFIXES), prefix_case([b"ab"] * 300, "same_prefix"), long_prefix_case(), bad_queries_case()]
    out += [nq_case(nq) for nq in (0, 1, 63, 64, 65, 257, 1023, 1024, 1025)]
    out += [one_level_count_case(n) for n in SMALL_COUNTS]
    out += [residue_case(r) for r in range(8)]
    return out


def table_cases() -> list:
    """Records around S = 2, 64 and 2,048 splitters."""
    return [counted_case(n) for n in (2047, 2049, 4097)]


def grid_cases() -> list:
    return [candidates_case(c) for c in GRID_COUNTS]


def random_cases() -> list:
    return [random_case(seed) for seed in range(4)]


def bad_record_case() -> ScanCase:
    """(the case, the offending seq): a record outside the source in the last
    level, which the one prefix has no match in."""
    c = winners_case()
    far = c.levels[2][0].copy()
    far[1, 1] = len(c.src) - int(far[1, 0]) + 1      # the key ends one byte past the source
    seq = len(c.levels[0][0]) + len(c.levels[1][0]) + 1
    return ScanCase("bad_record", c.src, [c.levels[0], c.levels[1], (far, 0)], *fc.lay_queries([b"k.zero"])), seq


def unordered_case() -> ScanCase:
    """A level whose keys do not ascend (and one that does): offences at seq 2 and 4 of level 0."""
    c = mc.from_items("unordered", [(k, b"v" + k) for k in (b"m", b"q", b"b", b"x", b"x", b"a", b"zz", b"c")] +
                      [(k, b"w" + k) for k in (b"a", b"b", b"n", b"x", b"y")], cuts=(8,))
    return ScanCase("unordered", c.src, c.lists, *fc.lay_queries([b"", b"a", b"x", b"m", b"q", b"b", b"z", b"c", b""]))


def shuffled_case(seed: int) -> ScanCase:
    """random_case(seed) with the records of every level in random order: nothing ascends."""
    c = random_case(seed, nq=40)
    rng = np.random.default_rng(50 + seed)
    return ScanCase("shuffled%d" % seed, c.src, [(r[rng.permutation(len(r))], b) for r, b in c.levels], c.qsrc, c.queries)
