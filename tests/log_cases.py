"""Cases for the log writer's tests (tests/test_log_host.py and
tests/test_log_layout.py on the CPU, tests/test_gpu_log.py on the GPU): a source
blob, a [n, 4] record list into it (key_off, key_len, val_off or 2^64-1,
val_len), a transaction table, where to write, and the image the call must give,
built with the format oracle's FileWriter (oracle/zs_format.py) by the adds,
removes and commits the list stands for.  Every builder checks on the host that
its case has the property it is there for; no GPU is needed."""
import functools

import numpy as np

from oracle import zs_format as zf
from tests import pack_cases as pc
from tests import records_images as ri
from tests.images import EINVAL64, OVERFLOW, U64_MAX  # noqa: F401  (the log tests read them as lc.*)
from zeroskip_amd import zsfile

UUID = bytes(range(16, 32))
SHORT = zf.MAX_SHORT_VAL_LEN


class Case:
    """tx_end None: one transaction a record; prefix: the bytes of [0, at) for
    an append (at = len(prefix)); src_in_prefix: the source IS the prefix (the
    records point into the image the call appends to); big: an image of 16 MiB."""

    def __init__(self, name, src, recs, tx_end=None, prefix=b"", finalise=False, prev_crc=0, startidx=3, endidx=3,
                 src_in_prefix=False, big=False):
        self.name, self.src, self.prefix = name, bytes(src), bytes(prefix)
        self.recs = np.ascontiguousarray(np.asarray(recs, dtype=np.uint64).reshape(-1, 4))
        self.tx_end = None if tx_end is None else [int(e) for e in tx_end]
        self.at, self.finalise, self.prev_crc = len(self.prefix), finalise, prev_crc
        self.uuid, self.startidx, self.endidx = UUID, startidx, endidx
        self.src_in_prefix, self.big = src_in_prefix, big
        assert self.at == 0 or (self.at >= 40 and self.at % 8 == 0)
        assert not src_in_prefix or self.src == self.prefix

    @property
    def n(self):
        return len(self.recs)

    def ends(self):
        return list(range(1, self.n + 1)) if self.tx_end is None else self.tx_end

    @property
    def n_commits(self):
        return len(self.ends()) + (1 if self.finalise else 0)

    @functools.cached_property
    def writer(self):
        """The FileWriter after the case's adds, removes and commits."""
        w = zf.FileWriter(self.uuid, self.startidx)
        w.buf = bytearray(zf.header_bytes(self.uuid, self.startidx, self.endidx))
        if self.at:
            w.buf = bytearray(self.prefix)
            w.mf_crc32 = self.prev_crc
        pairs, b = ri.as_pairs(self.src, self.recs), 0
        for e in self.ends():
            for k, v in pairs[b:e]:
                w.remove(k) if v is None else w.add(k, v)
            w.commit()
            b = e
        assert b == self.n
        if self.finalise:
            w.finalise()
        return w

    @property
    def want(self) -> bytes:
        """The whole image, the prefix included."""
        return self.writer.image()


class Blob(pc.Blob):
    def rec(self, kl, vl, kres=None, vres=None):
        """A record of random bytes: key length kl, value length vl (None: a delete)."""
        ko = self.put(kl, kres)
        return (ko, kl, U64_MAX, 0) if vl is None else (ko, kl, self.put(vl, vres), vl)


def from_lengths(name, lens, seed=0, **kw):
    """(key length, value length or None) pairs, random bytes."""
    b = Blob(seed)
    recs = [b.rec(kl, vl) for kl, vl in lens]
    return Case(name, b.buf, recs, **kw)


def _span_starts_at(case, t, i):
    """Commit t's span starts at record i (checked in the oracle's image by its own walk)."""
    commits, end, why = zf.walk(case.want)
    recs, rc = ri.host_records(case.want, zsfile.ACTIVE)
    assert why == "end" and all(c["ok"] for c in commits) and len(recs) == case.n
    assert commits[t]["span_off"] == int(recs[i, 0]) - 24, (case.name, t, i)


def check_against_image(case, d, got: bytes):
    """A writer's result (host twin or device): image, words and optional
    outputs against the oracle's image and its listing."""
    want = case.want
    assert d["code"] == 0 and d["n"] == case.n and d["end"] == len(want), (case.name, d["code"], d["end"], len(want))
    assert got[:len(want)] == want, case.name
    assert d["written"] == len(want) - case.at and d["commits"] == case.n_commits
    # what the lister and the walk find in the bytes written (the prefix cut off: offsets shifted back)
    if case.at:
        tail = zf.header_bytes(case.uuid, 0, 0) + want[case.at:]
        shift = case.at - 40
    else:
        tail, shift = want, 0
    recs, rc = ri.host_records(tail, zsfile.ACTIVE)
    assert rc == zsfile.END and len(recs) == case.n, case.name
    live = recs[:, 2] != U64_MAX
    recs[:, 0] += np.uint64(shift)
    recs[live, 2] += np.uint64(shift)
    assert np.array_equal(np.asarray(d["new_recs"]).view(np.uint64).reshape(-1, 4), recs), case.name
    off, ln, rc, end = zsfile.walk(tail)
    assert rc == zsfile.END and end == len(tail) and len(off) == case.n_commits, case.name
    assert np.array_equal(np.asarray(d["span_off"]).view(np.uint64), off + np.uint64(shift)), case.name
    assert np.array_equal(np.asarray(d["span_len"]).view(np.uint64), ln), case.name
    assert d["long_commits"] == sum(1 for o, l in zip(off, ln) if tail[int(o + l)] == zf.REC_LONG_COMMIT)
    assert d["last_crc"] == case.writer.mf_crc32, case.name
    stored = int.from_bytes(want[-4:], "big") if case.n_commits else 0
    assert d["stored_crc"] == stored, case.name
    nc = case.n_commits
    with np.errstate(over="ignore"):
        bound = zsfile.device_log_bound(case.n, nc, int(case.recs[:, 1].sum()), int(case.recs[case.recs[:, 2] != U64_MAX, 3].sum()))
    assert bound + (case.at - 40 if case.at else 0) >= len(want), case.name


# ------------------------------------------------------------------ small cases
@functools.lru_cache(maxsize=None)
def earlier_image(finalise=False) -> bytes:
    """An image to append to: 40 + 3 transactions; its length is 8 mod 16
    without the finalise commit and 0 mod 16 with it."""
    c = from_lengths("earlier", [(3, 5), (8, None), (1, 0), (16, 40)], seed=21, tx_end=[2, 3, 4], finalise=finalise)
    assert len(c.want) % 16 == (0 if finalise else 8)
    return c.want


def empties():
    none = np.zeros((0, 4), np.uint64)
    out = [Case("empty_no_table", b"", none), Case("empty_table_of_none", b"", none, tx_end=[]),
           Case("empty_appended", b"", none, tx_end=[], prefix=earlier_image()),
           Case("three_empty_tx", b"", none, tx_end=[0, 0, 0]),
           Case("three_empty_tx_finalise", b"", none, tx_end=[0, 0, 0], finalise=True),
           Case("finalise_only_fresh", b"", none, tx_end=[], finalise=True),
           Case("finalise_only_append_prev_crc", b"", none, tx_end=[], prefix=earlier_image(), finalise=True,
                prev_crc=0xDEADBEEF)]
    assert out[0].want == out[1].want == zf.header_bytes(UUID, 3, 3) and out[2].want == earlier_image()
    assert len(out[3].want) == 64 and out[3].want[40:48] == out[3].want[48:56]
    # the stale register: the finalise-only commit depends on prev_crc
    assert out[6].want[-8:] != Case("x", b"", none, tx_end=[], prefix=earlier_image(), finalise=True).want[-8:]
    return out


def finalise_after_tx():
    c = from_lengths("finalise_after_tx", [(5, 9), (2, 30)], seed=22, tx_end=[2], finalise=True)
    commits, _, _ = zf.walk(c.want)
    # the stale-CRC word: a commit of no bytes that does not verify from 0, hashed from the span before
    assert len(commits) == 2 and commits[0]["ok"] and commits[1]["span_len"] == 0 and not commits[1]["ok"]
    return c


def alignment_grid(name="alignment_grid", **kw):
    """Key lengths 0, 1, 7, 8, 9 x value lengths 0, 1, 7, 8, 9 at all 8 source alignments."""
    b, recs = Blob(23), []
    for r in range(8):
        for kl in (0, 1, 7, 8, 9):
            for vl in (0, 1, 7, 8, 9):
                recs.append(b.rec(kl, vl, kres=r, vres=(3 * r + kl + 1) % 8))
    c = Case(name, b.buf, recs, **kw)
    live = c.recs
    assert len(recs) == 200 and set(live[:, 0] % 8) == set(range(8)) == set(live[:, 2] % 8)
    return c


def shared_bytes():
    s = pc.shared_bytes()
    return Case("shared_bytes", s.src, s.recs, tx_end=list(range(50, len(s.recs), 50)) + [len(s.recs)])


def tx_shapes():
    out = []
    for name, lens, last_del in (("delete_first", [(4, None), (5, 6), (7, 8)], 0),
                                 ("delete_middle_then_adds", [(5, 6), (4, None), (7, 8), (1, 1)], 1),
                                 ("delete_last", [(5, 6), (7, 8), (4, None)], 2),
                                 ("two_deletes", [(5, 6), (4, None), (7, 8), (9, None), (3, 3)], 3),
                                 ("all_deletes", [(4, None), (0, None), (9, None)], 2)):
        # a transaction before and one behind, so that D[] carries marks across transactions
        lens = [(2, None), (3, 3)] + lens + [(6, 6)]
        c = from_lengths("tx_" + name, lens, seed=24, tx_end=[2, len(lens) - 1, len(lens)])
        _span_starts_at(c, 0, 0)                 # delete, add: at the delete
        out.append(c)
        _span_starts_at(c, 1, 2 + last_del)
        _span_starts_at(c, 2, len(lens) - 1)     # the delete marks before do not reach into a later transaction
    lens = [(3, 4), (5, None), (6, 7), (8, 9), (1, None), (2, 2), (10, 20)]
    out.append(from_lengths("tx_of_one", lens[:1], seed=25, tx_end=[1]))
    out.append(from_lengths("tx_of_everything", lens, seed=25, tx_end=[len(lens)]))
    _span_starts_at(out[-1], 0, 4)
    out.append(from_lengths("tx_end_null", lens, seed=25))
    assert len(zf.walk(out[-1].want)[0]) == len(lens)
    out.append(from_lengths("tx_mixed_empty", lens, seed=25, tx_end=[0, 0, 2, 2, 5, 7, 7], finalise=True))
    return out


def long_keys():
    out = [from_lengths("key_65535", [(3, 3), (65535, 10), (2, None)], seed=26, tx_end=[3]),
           from_lengths("key_65536", [(3, 3), (65536, 10), (65535, None)], seed=26, tx_end=[2, 3])]
    assert out[0].want[40 + 56] == zf.REC_KEY and out[1].want[40 + 56] == zf.REC_LONG_KEY
    return out


def counts():
    """0 .. 130 and 4,095 / 4,096 / 4,097 records of 24 .. 120 bytes in
    transactions of 0 .. 4: records and commits straddle the tiles of 64, 4,096
    and 65,536 bytes, and the record blocks of 1,024 and their scans end inside,
    at and behind a block."""
    out = []
    for n in list(range(131)) + [4095, 4096, 4097]:
        rng = np.random.default_rng(1000 + n)
        lens = [(int(rng.integers(0, 40)), None if rng.integers(0, 5) == 0 else int(rng.integers(0, 50)))
                for _ in range(n)]
        ends, e = [], 0
        while e < n:
            e = min(n, e + int(rng.integers(0, 5)))
            ends.append(e)
        out.append(from_lengths("count_%d" % n, lens, seed=n, tx_end=ends if n % 3 else None if n else [],
                                finalise=n % 5 == 1))
    return out


def appends():
    out = []
    for fin in (False, True):
        pre = earlier_image(fin)
        c = from_lengths("append_at_%d_mod_16" % (len(pre) % 16), [(4, 4), (9, None), (30, 100), (0, 0)], seed=27,
                         tx_end=[1, 1, 4], prefix=pre, finalise=True, prev_crc=0x1234)
        assert c.want[:len(pre)] == pre and zf.walk(c.want)[2] == "end"
        out.append(c)
    return out


def src_in_out():
    """The records of the image itself logged again behind it."""
    pre = earlier_image()
    recs, rc = ri.host_records(pre, zsfile.ACTIVE)
    assert rc == zsfile.END and len(recs) == 4
    c = Case("src_inside_out", pre, recs[::-1].copy(), tx_end=[1, 4], prefix=pre, src_in_prefix=True)
    assert ri.as_pairs(c.want, ri.host_records(c.want, zsfile.ACTIVE)[0])[4:] == ri.as_pairs(pre, recs)[::-1]
    return c


def long_span_small_records():
    """One transaction of 4,101 records of about 4 KiB that share their source
    bytes: a span above 16,777,215 bytes, its 24-byte commit across a 64 KiB
    tile edge."""
    b = Blob(28)
    ko, vo = b.put(8), b.put(66000)
    recs = [(ko, 8, vo, 4096)] * 4100
    fill = (65536 - 8 - 40 - 4100 * 4144) % 65536
    fill += 65536 if fill < 40 else 0
    recs.append((ko, 0, vo, fill - 40))
    c = Case("long_span_small_records", b.buf, recs + [(ko, 3, U64_MAX, 0)], tx_end=[4101, 4102], big=True)
    at = 40 + 4100 * 4144 + fill
    assert at % 65536 == 65528 and c.want[at] == zf.REC_LONG_COMMIT and at - 40 > SHORT
    return c


@functools.lru_cache(maxsize=None)
def small_cases():
    """Every case but the three of 16 MiB values."""
    out = empties() + [finalise_after_tx(), from_lengths("single_kv", [(3, 16)], seed=29),
                       alignment_grid(), alignment_grid("alignment_grid_tx_of_7", tx_end=list(range(7, 200, 7)) + [200]),
                       shared_bytes()] + tx_shapes() + long_keys() + counts() + appends() + [src_in_out()]
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


@functools.lru_cache(maxsize=None)
def big_cases():
    """A transaction of one record with an 8-byte key: a value of 16,777,160
    bytes (span 16,777,208: short value, short commit), of 16,777,168 (span
    16,777,216: short value, long commit), of 16,777,216 (long value, long
    commit); the long span of many small records."""
    out = []
    for name, vl, span, vtype, ctype in (("span_16777208", 16777160, 16777208, zf.REC_VALUE, zf.REC_COMMIT),
                                         ("span_16777216", 16777168, 16777216, zf.REC_VALUE, zf.REC_LONG_COMMIT),
                                         ("value_16777216", 16777216, 16777264, zf.REC_LONG_VALUE, zf.REC_LONG_COMMIT)):
        c = from_lengths(name, [(8, vl)], seed=30, tx_end=[1], big=True)
        assert c.want[40 + 32] == vtype and c.want[40 + span] == ctype and zf.walk(c.want)[0][0]["span_len"] == span
        out.append(c)
    return out + [long_span_small_records()]


# -------------------------------------------------------------------- bad input
def bad_inputs():
    """(name, case, cap, [res[0], res[1], res[2]]): cap None = room for the
    image; the output and the optional arrays must stay untouched."""
    base = from_lengths("bad_base", [(3, 4), (5, None), (6, 7), (8, 9), (1, None), (2, 2), (10, 20)], seed=31,
                        tx_end=[2, 2, 5, 7])
    size, n = len(base.src), base.n

    def variant(name, changes=(), tx_end=base.tx_end):
        recs = base.recs.copy()
        for i, col, v in changes:
            recs[i, col] = v
        return Case(name, base.src, recs, tx_end=tx_end)

    big_key = Blob(32)
    ko = big_key.put(65536)
    out = [
        ("record_outside_source", variant("b1", [(3, 0, size - 7)]), None, [EINVAL64, 3, U64_MAX]),
        ("value_end_wraps", variant("b2", [(2, 2, U64_MAX - 2), (2, 3, 8)]), None, [EINVAL64, 2, U64_MAX]),
        ("two_bad_records", variant("b3", [(5, 1, size + 1), (6, 3, U64_MAX)]), None, [EINVAL64, 5, U64_MAX]),
        ("long_delete", Case("b4", big_key.buf, [(0, 3, 4, 4), (ko, 65536, U64_MAX, 0)], tx_end=[2]), None,
         [EINVAL64, 1, U64_MAX]),
        ("tx_end_descending", variant("b5", tx_end=[2, 5, 4, 7]), None, [EINVAL64, U64_MAX, 2]),
        ("tx_end_above_n", variant("b6", tx_end=[2, 2, 8, 7]), None, [EINVAL64, U64_MAX, 2]),
        ("tx_end_last_not_n", variant("b7", tx_end=[2, 2, 5, 6]), None, [EINVAL64, U64_MAX, 3]),
        ("tx_end_none_for_records", variant("b8", tx_end=[]), None, [EINVAL64, U64_MAX, 0]),
        ("bad_record_and_bad_table", variant("b9", [(4, 0, size + 1)], tx_end=[3, 1, 7]), None, [EINVAL64, 4, 1]),
        ("one_byte_short", base, len(base.want) - 1, [OVERFLOW, n, len(base.want)]),
        ("eight_bytes_short", base, len(base.want) - 8, [OVERFLOW, n, len(base.want)]),
        ("sizing_call", base, 0, [OVERFLOW, n, len(base.want)]),
    ]
    return base, out
