"""Every family of hashing kernels at real unaligned base addresses.

The data of a shape is uploaded once inside junk that is never zero
(devmem.dev_at) and the base residues (address mod 64) are slices of that one
buffer, so `base & 3`, `base & ~3` below the base and the bytes before and
after a record are what they claim to be.  Every output lies between canary
fences that are checked after every call.  Every call runs seeded, with seed
0 and raw; the expectation is the CPU oracle's CRC of each record, computed
once per (residue, shape) and shared by every kernel variant -- the seeded
and raw values follow from it by the shift identity that
tests/test_hash_edge_cases.py checks, and the first and last record of each
are checked against the oracle's seeded call itself.  The case lists and what
they reach: tests/hash_edge_cases.py, tests/test_hash_edge_cases.py (CPU)."""
import os

import numpy as np
import pytest
import torch

from oracle import oracle
from tests import devmem as dm
from tests import hash_edge_cases as hc
from zeroskip_amd import device as zd
from zeroskip_amd._lib import DEFAULT_TEAMS, QTEAM_DEFAULT, lib

pytestmark = pytest.mark.gpu

M32 = 0xFFFFFFFF
THREADS = min(16, os.cpu_count() or 1)
QDEAL, QFOLD = 1 << 25, 32          # zs::BatchDesc::opt bits (tests/test_gpu_parity.py)
XTEAM_DEFAULT = (1, 256 << 10)
MODES = (("seeded", hc.SEED, False), ("seed0", 0, False), ("raw", hc.RAW_REG, True))
ONE_LANE = "team_kernel<1>/short_kernel/burst_kernel"

_pool = []


def pool(n, salt=0):
    """n random bytes: a window of one 160 MB draw (the shapes are big, the draw is slow)."""
    if not _pool:
        _pool.append(np.random.default_rng(0x4ED6E5).integers(0, 256, (160 << 20) + 8192, dtype=np.uint8))
    at = salt % 8192
    assert n + at <= _pool[0].size
    return _pool[0][at:at + n]


def expect(c0: np.ndarray, lens) -> dict:
    """Seeded, seed-0 and raw expectations from the records' plain CRCs:
    crc(seed, d) = shift(seed, len) ^ crc(0, d), raw(reg, d) = ~crc(~reg, d)."""
    lens = np.broadcast_to(np.asarray(lens, dtype=np.uint64), c0.shape)
    ks = {int(L): (oracle.shift(hc.SEED, int(L)), oracle.shift(~hc.RAW_REG & M32, int(L))) for L in np.unique(lens)}
    k_seed = np.array([ks[int(L)][0] for L in lens], dtype=np.uint32)
    k_raw = np.array([ks[int(L)][1] for L in lens], dtype=np.uint32)
    return {"seeded": c0 ^ k_seed, "seed0": c0, "raw": ~(c0 ^ k_raw)}


def fixed_want(host: np.ndarray, stride, L, n) -> dict:
    """The three expectations of n records of L bytes at `stride` from host[0]."""
    c0 = oracle.batch(host, n=n, stride=stride, fixed_len=L, impl="hw", threads=THREADS if n * L > (1 << 20) else 1)
    want = expect(c0, L)
    for i in {0, n - 1}:
        rec = host[i * stride:i * stride + L]
        assert oracle.crc32c_hw(hc.SEED, rec) == want["seeded"][i]
        assert ~oracle.crc32c_hw(~hc.RAW_REG & M32, rec) & M32 == want["raw"][i]
    return want


class Out:
    """n CRCs between two fences, refilled with the canary before every call."""

    def __init__(self, n, dev):
        self.n = n
        self.whole, o = dm.fenced(4 * n, dev)
        self.t = o.view(torch.int32)

    def fresh(self) -> torch.Tensor:
        self.whole.fill_(dm.CANARY)
        return self.t

    def got(self, what) -> np.ndarray:
        return dm.inside(self.whole, 4 * self.n, what).view(np.uint32)


def outs_for(cache: dict, n, dev) -> Out:
    if n not in cache:
        cache[n] = Out(n, dev)
    return cache[n]


def fixed_mismatches(dd, stride, L, n, want, out: Out, what) -> list:
    """zscrc_device_fixed in the three modes into the fenced output: what differs from `want`."""
    bad = []
    for mode, seed, raw in MODES:
        zd.crc_fixed(dd, stride, L, n, seed=seed, out=out.fresh(), raw=raw)
        got = out.got(what + (mode,))
        wrong = np.nonzero(got != want[mode])[0]
        if wrong.size:
            bad.append(what + (mode, int(wrong.size), wrong[:6].tolist()))
    return bad


def kernel_name(dd, stride, L, n) -> str:
    return lib().zscrc_fixed_kernel(dd.data_ptr(), stride, L, n).decode()


# ---------------------------------------------------------------- 16-lane coalesced teams
DYN = ("qteam_dyn_kernel", "qteam_dyn_kernel+qfold_kernel")
QTEAM_VARIANTS = (("static", 0, None, ("qteam_kernel",)), ("dealt-parts", QDEAL, "3", DYN),
                  ("dealt-parts-P1", QDEAL, "1", DYN), ("dealt-parts-qfold", QDEAL | QFOLD, "3", DYN[1:]),
                  ("xor3-1", 4, None, ("qteam_kernel",)), ("xor3-2", 8, None, ("qteam_kernel",)))


def big_shape(gpu, stride, L, n, residues):
    """One upload of a big fixed-stride shape; per residue its device slice and expectations."""
    host = pool(stride * (n - 1) + L + 64, stride * 7 + L)
    whole, view = dm.dev_at(host, gpu, 0)
    return whole, [(r, view[r:], fixed_want(host[r:], stride, L, n)) for r in residues]


def qteam_mismatches(gpu, stride, L, n, residues=hc.RESIDUES, variants=QTEAM_VARIANTS) -> list:
    """Every qteam variant at every residue of one shape; the failures as
    (variant, stride, len, n, residue, mode, count, first indices)."""
    whole, per = big_shape(gpu, stride, L, n, residues)
    out, bad = Out(n, gpu), []
    saved = os.environ.get("ZSCRC_QDYN_P")
    lib().zscrc_set_qteam(1)
    try:
        for vname, opt, P, names in variants:
            lib().zscrc_set_opt(opt)
            os.environ.pop("ZSCRC_QDYN_P", None)
            if P:
                os.environ["ZSCRC_QDYN_P"] = P     # parts of P KiB: ragged first parts, many per record
            for r, dd, want in per:
                assert dd.data_ptr() % 64 == r
                assert kernel_name(dd, stride, L, n) in names, (vname, stride, L, n, r)
                bad += fixed_mismatches(dd, stride, L, n, want, out, (vname, stride, L, n, r))
    finally:
        lib().zscrc_set_qteam(QTEAM_DEFAULT)
        lib().zscrc_set_opt(0)
        os.environ.pop("ZSCRC_QDYN_P", None)
        if saved is not None:
            os.environ["ZSCRC_QDYN_P"] = saved
    return bad


@pytest.mark.parametrize("stride,L,n", hc.QTEAM_SHAPES, ids=lambda v: str(v))
def test_qteam_at_every_phase(gpu, stride, L, n):
    """qteam_kernel, qteam_dyn_kernel with parts of 3 and 1 steps, its
    qfold_kernel form and the XOR3 groupings, at twelve residues of each shape:
    lengths around two and three steps, where base & 3 puts the record's first
    dword across the step-0 / step-1 boundary (pad 1021..1023) or at the very
    start of step 0 (pad 1..3), partial last groups of four, stride slack."""
    assert not qteam_mismatches(gpu, stride, L, n)


TEAM16_VARIANTS = (("auto", -1, 0), ("two-level", 0, 0), ("ring1", 1, 0), ("ring2", 2, 0),
                   ("auto-xor3", -1, 16), ("two-level-xor3", 0, 16))


@pytest.mark.parametrize("stride,L,n", hc.TEAM16_SHAPES, ids=lambda v: str(v))
def test_team16_at_every_phase(gpu, stride, L, n):
    """team_kernel<16> (qteam off): each shape on the walk it gets by default,
    on each forced walk (zscrc_set_prefetch(16, 0 / 1 / 2)) and with the XOR3
    bit, at the same residues; odd strides give the records of one call every phase."""
    whole, per = big_shape(gpu, stride, L, n, hc.RESIDUES)
    out, bad = Out(n, gpu), []
    lib().zscrc_set_qteam(0)
    try:
        for vname, depth, opt in TEAM16_VARIANTS:
            lib().zscrc_set_prefetch(16, depth)
            lib().zscrc_set_opt(opt)
            for r, dd, want in per:
                assert dd.data_ptr() % 64 == r
                assert kernel_name(dd, stride, L, n) == "team_kernel<16>", (vname, r)
                bad += fixed_mismatches(dd, stride, L, n, want, out, (vname, stride, L, n, r))
    finally:
        lib().zscrc_set_prefetch(16, -1)
        lib().zscrc_set_opt(0)
        lib().zscrc_set_qteam(QTEAM_DEFAULT)
    assert not bad, bad[:8]


# ---------------------------------------------------------------- small shapes, residues 0..63
def by_len(cases) -> dict:
    d = {}
    for c in cases:
        d.setdefault(c[1], []).append(c)
    return d


def small_len(gpu, L, cases):
    """One upload for every case of length L; per case its device slice and expectations."""
    need = max(stride * (n - 1) + L for stride, _, n, _ in cases) + 64
    host = pool(need, 131 * L)
    whole, view = dm.dev_at(host, gpu, 0)
    return whole, [(c, view[c[3]:], fixed_want(host[c[3]:], c[0], L, c[2])) for c in cases]


def run_small(gpu, cases, name) -> list:
    outs, bad = {}, []
    for L, cs in by_len(cases).items():
        whole, per = small_len(gpu, L, cs)
        for (stride, _, n, r), dd, want in per:
            assert dd.data_ptr() % 64 == r
            assert kernel_name(dd, stride, L, n) == name, (stride, L, n, r)
            bad += fixed_mismatches(dd, stride, L, n, want, outs_for(outs, n, gpu), (stride, L, n, r))
    return bad


@pytest.mark.parametrize("group", range(len(hc.XTEAM_LEN_GROUPS)), ids=["len1-16", "len63-65", "len4089-4103",
                                                                        "len8189-8200"])
@pytest.mark.parametrize("family", ["xteam_kernel", "team_kernel<64>"])
def test_whole_wave_teams_at_every_residue(gpu, family, group):
    """xteam_kernel (forced down to 1 byte) and team_kernel<64> at every base
    residue 0..63: records of < 8 bytes, shorter than one step, one step and
    two steps plus or minus a few bytes (the first dword spilling into step 1,
    the first step clamped at base & ~3), 1..129 records -- the result stash
    of 64 empty, full and one over."""
    if family == "xteam_kernel":
        lib().zscrc_set_xteam(1, 1)
        lib().zscrc_set_teams(0, 1 << 20)
    else:
        lib().zscrc_set_xteam(0, XTEAM_DEFAULT[1])
        lib().zscrc_set_teams(0, 0)
    try:
        bad = run_small(gpu, hc.xteam_cases(hc.XTEAM_LEN_GROUPS[group]), family)
    finally:
        lib().zscrc_set_xteam(*XTEAM_DEFAULT)
        lib().zscrc_set_teams(*DEFAULT_TEAMS)
    assert not bad, bad[:8]


@pytest.mark.parametrize("third", range(3), ids=["len1-100", "len101-200", "len201-300"])
def test_two_lane_teams_at_every_residue(gpu, third):
    """team_kernel<2> forced onto every length 1..300, eight residues each
    (every phase; all 64 over the lengths), odd strides, 1..129 records."""
    lib().zscrc_set_small_team(2)
    try:
        bad = run_small(gpu, [c for c in hc.TEAM2_CASES if 100 * third < c[1] <= 100 * third + 100], "team_kernel<2>")
    finally:
        lib().zscrc_set_small_team(0)
    assert not bad, bad[:8]


@pytest.fixture(scope="module")
def g1_data(gpu):
    """The one-lane cases on the device with their expectations, shared by the eleven walks."""
    return [small_len(gpu, L, cs) for L, cs in by_len(hc.G1_CASES).items()]


@pytest.mark.parametrize("walk", hc.G1_WALKS, ids=lambda w: "walk%d" % w)
def test_one_lane_walks_at_every_residue(gpu, g1_data, walk):
    """Each one-lane-per-record walk (zscrc_set_prefetch(1, k): the default,
    team_kernel<1>'s rings, short_kernel, burst_kernel with bursts of 1, 2 and
    5 pieces) on lengths 1..130, 312 and 640: eight residues each, strides that
    give the records every phase, 1..1000 records; among them the records
    whose initial register reaches past their first 64-byte piece."""
    outs, bad = {}, []
    lib().zscrc_set_small_team(1)     # no two-lane teams on the aligned cases
    lib().zscrc_set_prefetch(1, walk)
    try:
        for whole, per in g1_data:
            for (stride, L, n, r), dd, want in per:
                assert dd.data_ptr() % 64 == r and kernel_name(dd, stride, L, n) == ONE_LANE
                bad += fixed_mismatches(dd, stride, L, n, want, outs_for(outs, n, gpu), (walk, stride, L, n, r))
    finally:
        lib().zscrc_set_prefetch(1, -1)
        lib().zscrc_set_small_team(0)
    assert not bad, bad[:8]


# ---------------------------------------------------------------- k batches in one launch
@pytest.mark.parametrize("stride,L", hc.MULTI_SHAPES, ids=lambda v: str(v))
def test_fixed_multi_each_base_at_its_own_residue(gpu, stride, L):
    """zscrc_device_fixed_multi over 1, 3 and 64 batches, every base 16-byte
    aligned (multi64_kernel / multi64d_kernel on 64-byte records) or each at
    its own residue (multi_kernel's piece walk), 1..4099 records, every
    zscrc_set_opt variant; the k outputs lie between fences in one buffer."""
    nmax = max(hc.MULTI_N)
    seg = (stride * (nmax - 1) + L + 64 + 63) // 64 * 64 + 64
    host = pool(seg * max(hc.MULTI_K) + 64, 977 * L)
    whole, view = dm.dev_at(host, gpu, 0)
    bad = []
    for plan in (0, 1):
        for k in hc.MULTI_K:
            at = [b * seg + r for b, r in enumerate(hc.multi_residues(k, plan))]
            bufs = [view[a:a + seg - 64] for a in at]
            assert [b.data_ptr() % 64 for b in bufs] == list(hc.multi_residues(k, plan))
            wants = [fixed_want(host[a:], stride, L, nmax) for a in at]
            for n in hc.MULTI_N:
                fence, outs = dm.fenced_many(4 * n, k, gpu)
                o32 = [o.view(torch.int32) for o in outs]
                for opt in hc.MULTI_OPTS:
                    lib().zscrc_set_opt(opt)
                    try:
                        for mode, seed, raw in MODES:
                            fence.fill_(dm.CANARY)
                            zd.crc_fixed_multi(bufs, stride, L, n, seed=seed, outs=o32, raw=raw)
                            got = dm.inside_many(fence, 4 * n, k, (plan, k, n, opt, mode))
                            for b in range(k):
                                if not np.array_equal(got[b].view(np.uint32), wants[b][mode][:n]):
                                    bad.append((plan, k, n, opt, mode, b))
                    finally:
                        lib().zscrc_set_opt(0)
    assert not bad, bad[:8]


# ---------------------------------------------------------------- spans
SPAN_CONFIGS = {"default": None, "xteam-dealt16": 16, "xteam-dealt4": 4, "xteam-static": 0}
SPANS_SEG = ((max(hc.SPAN_LENS) + 64 + 63) // 64 + 1) * 64


@pytest.fixture(scope="module")
def span_data(gpu):
    """Eight segments of random bytes in one upload; the plain CRC of a span, computed once."""
    host = pool(8 * SPANS_SEG + 64, 5)
    whole, view = dm.dev_at(host, gpu, 0)
    memo = {}

    def want(at, L):
        if (at, L) not in memo:
            memo[(at, L)] = expect(np.array([oracle.crc32c_hw(0, host[at:at + L])], np.uint32), L)
        return memo[(at, L)]
    assert want(3, 5)["seeded"][0] == oracle.crc32c_hw(hc.SEED, host[3:8])
    assert want(1, 16387)["raw"][0] == ~oracle.crc32c_hw(~hc.RAW_REG & M32, host[1:16388]) & M32
    return whole, view, want, host


@pytest.mark.parametrize("config", list(SPAN_CONFIGS))
def test_spans_at_every_residue(gpu, span_data, config):
    """zscrc_device_span at every residue 0..63 (empty, tiny, around the
    16 KiB split, many segments) and zscrc_device_spans over eight spans at
    eight different residues in one call (the one-launch form, and a list
    with short spans that takes a call each) -- by default and on
    xteam_kernel's span walk forced down to 4 KiB, dealt 16 / 4 per wave and static."""
    whole, view, want, host = span_data
    per_wave = SPAN_CONFIGS[config]
    old = lib().zscrc_set_xdeal(per_wave) if per_wave is not None else None
    if per_wave is not None:
        lib().zscrc_set_xteam(1, 4096)
    one, eight, bad = Out(1, gpu), Out(8, gpu), []
    try:
        for L in hc.SPAN_LENS:
            for r in hc.ALL64:
                for mode, seed, raw in MODES:
                    zd.crc_span(view, seed=seed, length=L, offset=r, out=one.fresh(), raw=raw)
                    if one.got((L, r, mode))[0] != want(r, L)[mode][0]:
                        bad.append((L, r, mode))
        for lens in (hc.SPANS8_LENS, hc.SPANS8_MIXED):
            for rot in range(8):
                offs = [i * SPANS_SEG + r for i, r in enumerate(hc.spans8_residues(rot))]
                assert sorted((view.data_ptr() + o) % 64 for o in offs) == sorted(hc.spans8_residues(rot))
                # seeded: one seed a span; the shift identity holds per seed, so these come from the oracle itself
                seeds = [(hc.SEED + 0x9E3779B9 * i) & M32 for i in range(8)]
                for mode, sd, raw in (("seed0", None, False), ("raw", [hc.RAW_REG] * 8, True),
                                      ("seeded", [hc.SEED] * 8, False)):
                    zd.crc_spans(view, offs, lens, seeds=sd, out=eight.fresh(), raw=raw)
                    got = eight.got((lens, rot, mode))
                    ref = np.array([want(o, L)[mode][0] for o, L in zip(offs, lens)], np.uint32)
                    if not np.array_equal(got, ref):
                        bad.append((lens, rot, mode, got.tolist(), ref.tolist()))
                if rot == 0:
                    zd.crc_spans(view, offs, lens, seeds=seeds, out=eight.fresh())
                    ref = [oracle.crc32c_hw(s, host[o:o + L]) for s, o, L in zip(seeds, offs, lens)]
                    if eight.got("own seeds").tolist() != ref:
                        bad.append(("own seeds", rot))
    finally:
        if per_wave is not None:
            lib().zscrc_set_xteam(*XTEAM_DEFAULT)
            lib().zscrc_set_xdeal(old)
    assert not bad, bad[:8]


# ---------------------------------------------------------------- variable batches
@pytest.mark.parametrize("bounded", [True, False], ids=["bounded", "unbounded"])
def test_batch_with_the_base_at_every_residue(gpu, bounded):
    """zscrc_device_batch_bounded with the base itself at residues 1..63 and
    the first record at offset 0, so lo = base & ~3 lies below the first
    record: tiny and short records under a bound; unbounded, 16-lane and
    whole-wave records cut into parts among them."""
    lens = np.array(hc.batch_lens(bounded), np.uint64)
    gaps = (np.arange(hc.BATCH_N, dtype=np.uint64) * 5) % 9
    offs = np.zeros(hc.BATCH_N, np.uint64)
    offs[1:] = np.cumsum(lens[:-1] + gaps[:-1])
    assert offs[0] == 0 and lens[0] > 0
    seeds = ((np.arange(hc.BATCH_N, dtype=np.uint64) * 0x9E3779B9 + hc.SEED) & M32).astype(np.uint32)
    host = pool(int(offs[-1] + lens[-1]) + 64, 9 + bounded)
    whole, view = dm.dev_at(host, gpu, 0)
    d_offs = torch.from_numpy(offs.astype(np.int64)).to(gpu)
    d_lens = torch.from_numpy(lens.astype(np.int64)).to(gpu)
    d_seeds = torch.from_numpy(seeds.view(np.int32)).to(gpu)
    out, bad = Out(hc.BATCH_N, gpu), []
    for r in range(1, 64):
        dd, h = view[r:], host[r:]
        assert dd.data_ptr() % 64 == r
        want = {"seeded": oracle.batch(h, offs, lens, seeds, impl="hw", threads=THREADS),
                "seed0": oracle.batch(h, offs, lens, impl="hw", threads=THREADS),
                "raw": ~oracle.batch(h, offs, lens, ~seeds, impl="hw", threads=THREADS)}
        for mode, sd, raw in (("seeded", d_seeds, False), ("seed0", None, False), ("raw", d_seeds, True)):
            zd.crc_batch(dd, d_offs, d_lens, sd, out=out.fresh(), raw=raw, max_len=hc.BATCH_BOUND if bounded else None)
            wrong = np.nonzero(out.got((r, mode)) != want[mode])[0]
            if wrong.size:
                bad.append((r, mode, wrong[:6].tolist(), lens[wrong[:6]].tolist()))
    assert not bad, bad[:8]
