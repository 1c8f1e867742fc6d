"""The model and the cases of the successor stage's tests (tests/test_next_host.py,
tests/test_next_args.py and tests/test_next_order.py on the CPU,
tests/test_gpu_next.py on the GPU).  The model knows nothing of cursors or
steps over levels: it fills a dictionary from the oldest level to the newest,
sorts the keys and takes one bisect per query; states, cursors, filler and all
twelve result words follow from walking that one sorted list -- the order of
Python's bytes is memcmp_raw.  Levels come from tests/merge_cases.py,
tests/find_cases.py and tests/scan_cases.py.  No GPU is needed."""
import struct
from bisect import bisect_left, bisect_right

import numpy as np

from tests import find_cases as fc
from tests import merge_cases as mc
from tests import scan_cases as sc

U64_MAX = fc.U64_MAX
EINVAL64 = fc.EINVAL64
NONE = fc.NONE
RES_WORDS = 12
PAGE, END, MORE, BAD = 0, 1, 2, 3
INCLUSIVE, CHECK_ORDER, KEEP_DELETES = 1, 2, 4
recs_of = fc.recs_of
NO_COMPARE = "no expected rows"
FILLER = (NONE, 0, 0, 0)


def merged(src: bytes, levels):
    """(the keys of all levels sorted, key -> (the winning record rebased, its
    seq, the levels that hold the key))."""
    src = bytes(src)
    levels = [(recs_of(r), int(b)) for r, b in levels]
    firsts = np.cumsum([0] + [len(r) for r, _ in levels])
    newest = {}
    for l in reversed(range(len(levels))):
        recs, base = levels[l]
        for j, key in enumerate(fc.level_keys(src, recs, base)):
            ko, kl, vo, vl = (int(v) for v in recs[j])
            copies = newest[key][2] if key in newest else 0
            newest[key] = ((ko + base, kl, vo if vo == U64_MAX else vo + base, vl), int(firsts[l]) + j, copies + 1)
    return sorted(newest), newest


def model(src: bytes, levels, qsrc: bytes, queries, page=1, inclusive=False, keep_deletes=False, max_steps=0,
          table=None):
    """(rows uint64 [nq, page, 4], seqs [nq, page], cur [nq, 4], the twelve
    result words) for levels = [(recs, base)] whose records lie inside src and
    ascend.  table: merged(src, levels), if at hand."""
    qsrc = bytes(qsrc)
    keys, newest = table or merged(src, levels)
    queries = recs_of(queries)
    nq = len(queries)
    rows = np.empty((nq, page, 4), np.uint64)
    rows[:] = np.asarray(FILLER, np.uint64)
    seqs = np.full((nq, page), U64_MAX, np.uint64)
    cur = np.zeros((nq, 4), np.uint64)
    res = [0, nq] + [0] * (RES_WORDS - 2)
    for i, (off, ln) in enumerate(queries[:, :2].tolist()):
        if off > len(qsrc) or ln > len(qsrc) - off:
            res[6] += 1
            cur[i] = (NONE, 0, 0, BAD)
            continue
        q = qsrc[off:off + ln]
        pos = bisect_left(keys, q) if inclusive else bisect_right(keys, q)
        count, steps, last = 0, 0, (NONE, 0)
        while True:
            if count == page:
                state = PAGE
                break
            if pos == len(keys):
                state, last = END, (NONE, 0)
                break
            if max_steps and steps == max_steps:
                state = MORE
                break
            row, seq, copies = newest[keys[pos]]
            pos += 1
            steps += 1
            last = row[:2]
            res[4] += copies - 1
            dele = row[2] == U64_MAX
            res[5] += dele
            if dele and not keep_deletes:
                continue
            rows[i, count], seqs[i, count] = row, seq
            count += 1
            res[8] += row[1]
            res[9] += 0 if dele else row[3]
        cur[i] = (last[0], last[1], count, state)
        res[2] += count
        res[3] += steps
        res[10] += state == END
        res[11] += state == MORE
    return rows, seqs, cur, res


class NextCase:
    """src, levels [(recs, base)], the query blob and the queries."""

    def __init__(self, name, src, levels, qsrc, queries):
        self.name, self.src, self.qsrc = name, bytes(src), bytes(qsrc)
        self.levels = [(recs_of(r), int(b)) for r, b in levels]
        self.queries = recs_of(queries)
        self._table, self._model = None, {}

    def model(self, page=1, inclusive=False, keep_deletes=False, max_steps=0):
        """Computed once a setting and shared: treat the arrays as read-only."""
        key = (page, inclusive, keep_deletes, max_steps)
        if key not in self._model:
            if self._table is None:
                self._table = merged(self.src, self.levels)
            self._model[key] = model(self.src, self.levels, self.qsrc, self.queries, page, inclusive, keep_deletes,
                                     max_steps, self._table)
        return self._model[key]

    @property
    def n(self):
        return sum(len(r) for r, _ in self.levels)

    def case_file(self, page=1, inclusive=False, keep_deletes=False, max_steps=0, shift=0, qshift=0, want=None) -> bytes:
        """The case as tests/c/next_order.cpp reads it; want = NO_COMPARE: no
        expected words, the program only runs and checks its positions."""
        recs = np.concatenate([r for r, _ in self.levels]) if self.levels else recs_of([])
        body = b"".join(struct.pack("<2Q", len(r), b) for r, b in self.levels) + self.src + recs.tobytes() + \
            self.qsrc + self.queries.tobytes()
        compare = want is not NO_COMPARE
        if compare:
            rows, seqs, cur, res = self.model(page, inclusive, keep_deletes, max_steps) if want is None else want
            body += b"".join(np.ascontiguousarray(a, np.uint64).tobytes() for a in (rows, seqs, cur, res))
        flags = (INCLUSIVE if inclusive else 0) | (KEEP_DELETES if keep_deletes else 0)
        return struct.pack("<11Q", len(self.src), len(self.levels), len(recs), len(self.qsrc), len(self.queries), shift,
                           qshift, page, flags, max_steps, int(compare)) + body


def all_keys(src, levels) -> list:
    return sorted({k for r, b in levels for k in fc.level_keys(src, recs_of(r), int(b))})


def probes(keys, step=1) -> list:
    """Of every step-th key: the key, the key with a zero byte and with 0xff
    appended; the first and the last key whatever the step, the empty key, one
    key below the first and one above the last."""
    keys = list(keys)
    out = [b""]
    for k in keys[::step] + keys[:1] + keys[-1:]:
        out += [k, k + b"\x00", k + b"\xff"]
    if keys:
        lo, hi = keys[0], keys[-1]
        out += [lo[:-1], hi + b"\xff\xff"]
        if lo and lo[-1]:
            out.append(lo[:-1] + bytes([lo[-1] - 1]))
    return out


def over(name, src, levels, step=1, residue=None, extra=()) -> NextCase:
    """The levels under probes of their own keys."""
    return NextCase(name, src, levels, *fc.lay_queries(probes(all_keys(src, levels), step) + list(extra), residue))


def from_scan(c: sc.ScanCase, step=1) -> NextCase:
    """A scan case's levels under probes of their keys, and under its prefixes as keys."""
    pre = [c.qsrc[int(o):int(o) + int(n)] for o, n in c.queries[:40, :2] if int(o) + int(n) <= len(c.qsrc)]
    return over(c.name, c.src, c.levels, step, extra=pre)


def from_items(name, items, queries, cuts=(), residue=None, qresidue=None) -> NextCase:
    c = mc.from_items(name, items, cuts=cuts, residue=residue)
    return NextCase(name, c.src, fc.split_levels(c), *fc.lay_queries(queries, qresidue))


def five_levels_case() -> NextCase:
    """k = 5: three levels that share keys, an empty one first and one between."""
    items = [(b"k%02d" % i, b"a%d" % i) for i in range(0, 30, 2)] + \
            [(b"k%02d" % i, None if i % 9 == 0 else b"b%d" % i) for i in range(0, 30, 3)] + \
            [(b"k%02d" % i, b"c%d" % i) for i in range(30)]
    c = mc.from_items("five_levels", items, cuts=(15, 25))
    l0, l1, l2 = fc.split_levels(c)
    return over("five_levels", c.src, [(recs_of([]), 5), l0, l1, (recs_of([]), 0), l2])


def every_level_case() -> NextCase:
    """One key present in all 64 levels, each level with a key of its own before or after it."""
    items, cuts = [], []
    for l in range(64):
        own = (b"a%02d" % l, b"own%d" % l) if l % 2 else (b"z%02d" % l, None if l % 8 == 0 else b"own%d" % l)
        items += sorted([own, (b"shared", None if l == 0 else b"s%d" % l)])
        cuts.append(len(items))
    c = mc.from_items("every_level", items, cuts=cuts[:-1])
    return over("every_level", c.src, fc.split_levels(c), step=7, extra=[b"shared", b"share", b"shared\x00"])


def run_items(run: int):
    """A value, `run` consecutive winning deletes, two values; an older level
    holds a value under every third of the deleted keys."""
    new = [(b"a", b"first")] + [(b"d%04d" % i, None) for i in range(run)] + [(b"y", b"after"), (b"z", b"last")]
    old = [(b"d%04d" % i, b"old%d" % i) for i in range(0, run, 3)] + [(b"y", b"older")]
    return new + old, len(new)


def delete_run_case(run: int) -> NextCase:
    items, cut = run_items(run)
    return from_items("run%d" % run, items, [b"a", b"", b"d0000", b"y", b"z"], cuts=(cut,))


DELETE_RUNS = (0, 1, 2, 63, 64, 65, 1000)


def run_steps(run: int) -> list:
    """max_steps at 1 and around the run's length."""
    return sorted({s for s in (1, run - 1, run, run + 1) if s > 0})


def inclusive_case() -> NextCase:
    """Queries on a live key, on a deleted key and on an absent key (sc.winners_case's levels)."""
    c = sc.winners_case()
    return NextCase("inclusive", c.src, c.levels, *fc.lay_queries(
        [b"k.every", b"k.zero", b"k.del-over-value", b"k.mid", b"k.value-over-del", b"k.absent", b"k.", b"", b"l"]))


def bad_queries_case() -> NextCase:
    c = from_scan(sc.prefix_case(sc.PREFIXES))
    q = c.queries.copy()
    q[1] = (len(c.qsrc) + 1, 0, 0, 0)            # starts past the end
    q[2] = (len(c.qsrc) - 1, 2, 0, 0)            # ends one byte past it
    q[4] = (U64_MAX, 1, 0, 0)
    q[7] = (NONE, 0, 0, END)                     # an END cursor fed again
    return NextCase("bad_queries", c.src, c.levels, c.qsrc, q)


def nq_case(nq: int) -> NextCase:
    c = sc.prefix_case([b""])
    q = (probes(all_keys(c.src, c.levels)) * (nq // 40 + 1))[:nq]
    return NextCase("nq%d" % nq, c.src, c.levels, *fc.lay_queries(q))


def level_size_case(n: int) -> NextCase:
    """One level of n records over an older one of every other of them."""
    src, recs = fc.counted_level(n)
    return over("size%d" % n, src, [(recs, 0), (recs[::2].copy(), 0)], step=max(1, n // 9))


def residue_case(r: int) -> NextCase:
    c = sc.residue_case(r)
    return over("residue%d" % r, c.src, c.levels, step=3, residue=(r + 3) % 8)


def random_case(seed: int) -> NextCase:
    f = fc.random_find_case(seed, nq=150)
    return NextCase("random%d" % seed, f.src, f.levels, f.qsrc, f.queries)


NQ_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257)
LEVEL_SIZES = (1, 2, 3, 1023, 1024, 1025, 2047, 2048, 2049)      # 1, and S - 1, S, S + 1 for S = 2, 1,024 and 2,048
PAGES = (1, 2, 3, 64)


def small_cases() -> list:
    """The cases every implementation is held against."""
    by_name = {c.name: c for c in mc.small_cases()}
    out = [NextCase("no_levels", b"", [], *fc.lay_queries([b"", b"k"])),
           NextCase("empty_levels", b"abc", [(recs_of([]), 0)] * 3, *fc.lay_queries([b"", b"k", b"abc"]))]
    out += [from_scan(sc.counted_case(n), max(1, n // 9)) for n in (0, 1, 2, 3, 63, 64, 65)]
    out += [from_scan(sc.many_levels_case()), five_levels_case(), every_level_case(), inclusive_case()]
    out += [from_scan(sc.winners_case()), from_scan(sc.deletes_case()), from_scan(sc.twice_case(), 40)]
    out += [from_scan(sc.prefix_case(sc.PREFIXES)), bad_queries_case()]
    for n in ("shared_prefix", "key_lengths", "ends_at_last_byte"):      # keys of 0 to 17 bytes, equal past byte 16
        f = fc.one_level(by_name[n])
        out.append(over(n, f.src, f.levels + [(f.levels[0][0][::3].copy(), 0)]))
    out += [delete_run_case(run) for run in DELETE_RUNS if run <= 65]
    out += [nq_case(nq) for nq in NQ_COUNTS]
    out += [residue_case(r) for r in range(8)]
    return out


def settings(case) -> list:
    """(page, inclusive, keep_deletes, max_steps) a small case is run at: every
    page size and every flag, not their whole product."""
    out = [(1, False, False, 0), (2, True, False, 0), (3, False, True, 0), (64, True, True, 0), (64, False, False, 0),
           (3, False, False, 1), (2, True, True, 2)]
    if case.name.startswith("run"):
        run = int(case.name[3:])
        out += [(p, False, keep, s) for s in run_steps(run) for p, keep in ((1, False), (64, False), (2, True))]
    return out


def table_cases() -> list:
    return [level_size_case(n) for n in LEVEL_SIZES]


def random_cases() -> list:
    return [random_case(seed) for seed in range(4)]


def bad_record_case():
    """(the case, the offending seq): a record outside the source in the last level."""
    c, seq = sc.bad_record_case()
    return NextCase("bad_record", c.src, c.levels, *fc.lay_queries([b"k.zero", b""])), seq


def unordered_case() -> NextCase:
    """A level whose keys do not ascend (and one that does): offences at seq 2 and 4 of level 0."""
    c = sc.unordered_case()
    return over("unordered", c.src, c.levels)


def shuffled_case(seed: int) -> NextCase:
    c = sc.shuffled_case(seed)
    return over("shuffled%d" % seed, c.src, c.levels, step=25)

