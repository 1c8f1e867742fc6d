"""Cases for the device merge's tests (tests/test_merge_order.py on the CPU,
tests/test_gpu_merge.py on the GPU): a source blob, record lists into it
([n, 4] uint64: key_off, key_len, val_off or 2^64-1, val_len) each with the
base that is added to its offsets, and the list the merge must give -- the
few lines of Python of model().  No GPU is needed."""
import struct

import numpy as np

from tests.images import OVERFLOW, U64_MAX  # noqa: F401  (the tests read them as mc.*)


class Case:
    def __init__(self, name, src, lists):
        self.name, self.src = name, bytes(src)
        self.lists = [(np.ascontiguousarray(np.asarray(r, dtype=np.uint64).reshape(-1, 4)), int(b)) for r, b in lists]

    @property
    def n(self):
        return sum(len(r) for r, _ in self.lists)

    def rebased(self) -> np.ndarray:
        """The concatenation of the lists, every offset with its list's base added."""
        out = []
        for r, b in self.lists:
            r = r.copy()
            r[:, 0] += np.uint64(b)
            live = r[:, 2] != U64_MAX
            r[live, 2] += np.uint64(b)
            out.append(r)
        return np.concatenate(out) if out else np.zeros((0, 4), np.uint64)

    def keys(self) -> list:
        return [self.src[int(o):int(o) + int(ln)] for o, ln in self.rebased()[:, :2]]

    def model(self, drop_deletes: bool):
        """(the winners in key order [m, 4], the eight result words)."""
        recs, key = self.rebased(), self.keys()
        n = len(recs)
        ordered = sorted(range(n), key=lambda i: (key[i], i))
        last = [i for p, i in enumerate(ordered) if p + 1 == n or key[ordered[p + 1]] != key[i]]
        dele = [i for i in last if int(recs[i, 2]) == U64_MAX]
        win = [i for i in last if not (drop_deletes and int(recs[i, 2]) == U64_MAX)]
        w = recs[win].reshape(-1, 4)
        live = w[w[:, 2] != U64_MAX]
        res = [0, len(win), n, 0 if drop_deletes else len(dele), int(w[:, 1].sum(dtype=np.uint64)),
               int(live[:, 3].sum(dtype=np.uint64)), n - len(last), len(dele) if drop_deletes else 0]
        return w, res

    def pairs(self, recs) -> list:
        """[(key, value-or-None)] of rebased records."""
        s = self.src
        return [(s[int(ko):int(ko) + int(kl)], None if int(vo) == U64_MAX else s[int(vo):int(vo) + int(vl)])
                for ko, kl, vo, vl in recs]

    def case_file(self, shift: int, drop_deletes: bool, want=None) -> bytes:
        """The case as tests/c/merge_order.cpp reads it."""
        want = self.model(drop_deletes)[0] if want is None else want
        recs = np.concatenate([r for r, _ in self.lists]) if self.lists else np.zeros((0, 4), np.uint64)
        head = struct.pack("<6Q", len(self.src), len(self.lists), len(recs), len(want), shift, int(drop_deletes))
        return head + b"".join(struct.pack("<2Q", len(r), b) for r, b in self.lists) + self.src + recs.tobytes() + \
            np.ascontiguousarray(want, np.uint64).tobytes()


def from_items(name, items, cuts=(), residue=None, pad_end=True, seed=0):
    """items: (key, value or None) in input order, keys and values laid one
    after another into a blob (each key at offset = residue mod 8 if given,
    values of a few bytes); cuts: the input positions at which a new list
    starts.  One blob, every base 0."""
    buf, recs = bytearray(), []
    for k, v in items:
        if residue is not None:
            buf += b"\xEE" * ((residue - len(buf)) % 8)
        ko = len(buf)
        buf += k
        if v is None:
            recs.append((ko, len(k), U64_MAX, 0))
        else:
            recs.append((ko, len(k), len(buf), len(v)))
            buf += v
    if pad_end:
        buf += b"\xEE" * 3
    recs = np.asarray(recs, dtype=np.uint64).reshape(-1, 4)
    edges = [0] + list(cuts) + [len(recs)]
    return Case(name, buf, [(recs[a:b], 0) for a, b in zip(edges[:-1], edges[1:])])


def _val(i):
    return b"v%d" % i


def counted(n, seed=1):
    """n records of 12-byte keys in random order: `key-` + 8 digits, a tenth of them repeated."""
    rng = np.random.default_rng(seed + n)
    ids = rng.integers(0, max(1, n - n // 10), n)
    return from_items("n%d" % n, [(b"key-%08d" % int(k), _val(i)) for i, k in enumerate(ids)])


def shared_prefix():
    """Keys that share their first 8 bytes (and more) and differ at byte 8, 9, 15, 16 or 17."""
    stem = b"PREFIX--" + b"m" * 12
    items = []
    for at in (8, 9, 15, 16, 17):
        for c in (b"a", b"z", b"\x00", b"\xff", b"m"):
            k = stem[:at] + c + stem[at + 1:]
            items += [(k, _val(len(items))), (k[:at + 1], _val(len(items) + 1))]
    return from_items("shared_prefix", items[::-1] + items[::3])


def key_lengths():
    """Prefixes of one another from b"" to b"a" + 9 zero bytes, the same with
    a trailing 0x01, bytes >= 0x80 against bytes < 0x80, a key of length 0."""
    keys = [b"", b"a"] + [b"a" + bytes(z) for z in range(1, 10)] + [b"a" + bytes(z) + b"\x01" for z in range(0, 10)]
    keys += [b"\x7f", b"\x80", b"\xff", b"a\x7fz", b"a\x80", b"a\xff\x00", b"abcdefgh\x7f", b"abcdefgh\x80",
             b"abcdefgh", b"abcdefg", b"abcdefghi", b"abcdefgh\x00", b"abcdefghabcdefgh\x80", b"abcdefghabcdefgh\x7f\xff"]
    items = [(k, _val(i)) for i, k in enumerate(keys)]
    rng = np.random.default_rng(3)
    order = rng.permutation(len(items))
    return from_items("key_lengths", [items[i] for i in order] + items[::-1][::2])


def residues(r):
    """Keys of 0..19 bytes, each at source offset r mod 8."""
    rng = np.random.default_rng(40 + r)
    items = []
    for ln in range(20):
        for _ in range(3):
            items.append((rng.integers(97, 100, ln, dtype=np.uint8).tobytes(), _val(len(items))))
    return from_items("residue%d" % r, items, residue=r)


def ends_at_last_byte():
    """The last key ends with the source's last byte; an empty key lies at src_size."""
    c = from_items("ends_at_last_byte", [(b"zz-the-last-key-of-all", None), (b"aa", b"1"), (b"zz-the-last-key-of-alm", b"2"),
                                        (b"zz-the-last-key-of-all", None)], pad_end=False)
    src = c.src
    recs = np.concatenate([c.lists[0][0], np.asarray([(len(src), 0, U64_MAX, 0)], dtype=np.uint64)])
    assert int(recs[3, 0] + recs[3, 1]) == len(src)
    return Case("ends_at_last_byte", src, [(recs, 0)])


def long_keys():
    """Two 70,000-byte keys that differ in their last byte only, the greater one first."""
    stem = np.random.default_rng(5).integers(0, 256, 69999, dtype=np.uint8).tobytes()
    return from_items("long_keys", [(stem + b"\x81", b"big"), (b"q", b"small"), (stem + b"\x80", b"BIG")])


def one_key(n=500):
    return from_items("one_key", [(b"the-same-key", None if i % 7 == 3 else _val(i)) for i in range(n)])


def sorted_and_reversed():
    items = [(b"k%09d" % i, _val(i)) for i in range(700)]
    return [from_items("sorted", items), from_items("reversed", items[::-1])]


def one_and_thousand():
    """Two sorted lists of 1 and 1,000 records, the shape of two packed files."""
    big = [(b"user.%06d" % (3 * i), _val(i)) for i in range(1000)]
    return from_items("one_and_thousand", [(b"user.000300", None)] + big, cuts=(1,))


def deletes():
    """A delete over an earlier value and a value over an earlier delete, in one list and across lists."""
    items = [(b"a", b"1"), (b"b", None), (b"c", b"3"), (b"d", None), (b"a", None), (b"b", b"2"), (b"e", None),
             (b"c", None), (b"d", b"4"), (b"f", b"6"), (b"e", None)]
    return from_items("deletes", items, cuts=(4, 7))


def twice():
    """One list passed twice with two bases into an arena that holds the same image twice."""
    c = counted(300, seed=9)
    img = c.src + b"\xEE" * (-len(c.src) % 64)
    recs = c.lists[0][0]
    return Case("twice", img + img, [(recs, 0), (recs, len(img))])


def random_case(seed, n=2000):
    """n records over 1-4 lists, keys of 0-20 letters from a 3-letter alphabet, one in five a delete."""
    rng = np.random.default_rng(1000 + seed)
    items = []
    for i in range(n):
        k = rng.integers(97, 100, int(rng.integers(0, 21)), dtype=np.uint8).tobytes()
        items.append((k, None if rng.integers(0, 5) == 0 else _val(i)))
    nl = int(rng.integers(1, 5))
    cuts = sorted(int(c) for c in rng.integers(0, n + 1, nl - 1))
    return from_items("random%d" % seed, items, cuts=cuts)


def small_cases():
    out = [Case("no_lists", b"", []), Case("empty_lists", b"abc", [(np.zeros((0, 4), np.uint64), 0)] * 3),
           from_items("one_record", [(b"only", b"one")])]
    out += [counted(n) for n in (63, 64, 65, 129, 192, 320, 255, 256, 257, 513, 768, 1280)]
    out += [shared_prefix(), key_lengths()] + [residues(r) for r in range(8)]
    out += [ends_at_last_byte(), long_keys(), one_key()] + sorted_and_reversed()
    out += [one_and_thousand(), deletes(), twice()]
    return out
