"""tests/hash_edge_cases.py: the case lists of tests/test_gpu_hash_edges.py
reach the branches of the hashing kernels they were chosen for, by the
kernels' own geometry formulas restated there; and the two oracles the GPU
tests' expectations rest on agree.  No GPU."""
import numpy as np

from oracle import oracle
from tests import hash_edge_cases as hc

BASE = 1 << 20   # any 64-byte aligned address: only base mod 64 enters the geometry


def test_qteam_geom_is_qgeoms_arithmetic():
    assert hc.qteam_geom(0, 8192) == (0, 8192, 8, 0, 0)
    assert hc.qteam_geom(1, 8195) == (1, 8195, 9, 1021, 0)
    assert hc.qteam_geom(2, 2050) == (2, 2050, 3, 1022, 0)
    assert hc.qteam_geom(3, 2049) == (3, 2049, 3, 1023, 0)
    assert hc.qteam_geom(3, 2050) == (3, 2049, 3, 1023, 1)
    assert hc.qteam_geom(0, 2051) == (0, 2048, 2, 0, 3)
    for r in hc.ALL64:
        for L in (1024, 2047, 2048, 2049, 3071, 8195):
            ph, span, S, pad, tail = hc.qteam_geom(r, L)
            assert ph == r % 4 and (r + span) % 4 == 0 and 0 <= tail < 4 and span + tail == L
            assert 0 <= pad < 1024 and (S * 1024 - pad) == span and pad % 4 == ph


def test_qteam_list_reaches_the_step_1_fixup_and_every_phase():
    cases = hc.QTEAM_CASES
    geom = {(s, L, n, r): hc.qteam_geom(r, L) for s, L, n, r in cases}
    pads = {(g[0], g[3]) for g in geom.values()}
    # pad > 1020 ("its first 4 bytes reach step 1"): pad = phase mod 4, so 1020 + phase
    for ph in (1, 2, 3):
        assert (ph, 1020 + ph) in pads
        assert (ph, ph) in pads                                   # pad < 4: the record starts in step 0's first dword
        assert any(g[0] == ph and g[3] > 1020 and r >= 16 for (_, _, _, r), g in geom.items())
        assert any(g[0] == ph and g[3] > 1020 and r >= 48 for (_, _, _, r), g in geom.items())
        assert {t for (p, _, _, _, t) in geom.values() if p == ph} == {0, 1, 2, 3}   # every tail
    assert (0, 0) in pads and not any(p > 1020 for ph, p in pads if ph == 0)
    assert geom[(8200, 8195, 16385, 1)][3] == 1021 and geom[(3000, 2050, 16387, 2)][3] == 1022
    for ph in (0, 1, 2, 3):
        rs = [r for r in hc.RESIDUES if r % 4 == ph]
        assert any(r < 16 for r in rs) and any(16 <= r for r in rs) and any(r >= 48 for r in rs)
    # what the kernels and team_for ask of a qteam shape; partial last groups; every stride slack
    slack = set()
    for stride, L, n in hc.QTEAM_SHAPES:
        assert stride % 4 == 0 and stride >= L and L >= 2048 and n >= 16384
        slack.add(stride - ((L + 3) & ~3))
    assert {0, 4, 64} <= slack and {n % 4 for _, _, n in hc.QTEAM_SHAPES} == {0, 1, 3}
    assert {(n, s - ((L + 3) & ~3)) for s, L, n in hc.QTEAM_SHAPES[:18]} == {(n, a) for n in hc.QTEAM_N
                                                                           for a in (0, 4, 64)}
    assert max(s * n for s, _, n in hc.QTEAM_SHAPES[:18]) < 56 << 20


def test_team16_list_takes_every_walk():
    lens = [L for _, L, _ in hc.TEAM16_SHAPES]
    assert any(700 <= L <= 2048 for L in lens) and any(2049 <= L <= 8191 for L in lens)
    assert sum(L >= 8192 for L in lens) >= 3 and any(s % 2 for s, _, _ in hc.TEAM16_SHAPES)
    assert all(n >= 16384 and s >= L > 640 for s, L, n in hc.TEAM16_SHAPES)
    # with STEP = 1024: first 4 bytes reaching step 1, at some residue of the set
    spill = [(L, r) for _, L, _ in hc.TEAM16_SHAPES for r in hc.RESIDUES
             for E, S, V0, _ in [hc.step_geom(BASE + r, L, 1024)] if (r & 3) and V0 + 1024 < BASE + r + 4]
    assert spill


def test_xteam_list_reaches_spills_clamps_and_short_records():
    cases = hc.XTEAM_CASES
    assert len(cases) == 64 * sum(len(g) for g in hc.XTEAM_LEN_GROUPS)
    spill = clamp = short = tiny = 0
    for stride, L, n, r in cases:
        for i in {0, 1, n - 1}:
            A = BASE + r + i * stride
            lo = (BASE + r) & ~3
            E, S, V0, tail = hc.step_geom(A, L, hc.XSTEP)
            assert V0 <= A and E <= A + L and 0 <= tail < 8
            spill += (A & 3) != 0 and S >= 2 and V0 + hc.XSTEP < A + 4
            clamp += A - lo < 64 and S >= 1 and V0 < lo
            short += 8 <= L < hc.XSTEP
            tiny += L < 8
    assert spill >= 9 and clamp >= 64 and short and tiny
    # every (n, stride slack) pair, every residue at every length
    assert {(n, s - L) for s, L, n, _ in cases} == {(n, a) for n in hc.XTEAM_N for a in (0, 1)}
    assert {(L, r) for _, L, _, r in cases} == {(L, r) for g in hc.XTEAM_LEN_GROUPS for L in g for r in hc.ALL64}


def test_spread8_gives_each_length_every_phase_and_the_list_every_residue():
    for L in range(1, 400):
        rs = hc.spread8(L)
        assert sorted(r % 4 for r in rs) == [0, 0, 1, 1, 2, 2, 3, 3] and len(set(rs)) == 8
    assert {r for _, _, _, r in hc.TEAM2_CASES} == set(hc.ALL64)
    assert {r for _, _, _, r in hc.G1_CASES} == set(hc.ALL64)
    assert {L for _, L, _, _ in hc.TEAM2_CASES} == set(range(1, 301))
    assert {L for _, L, _, _ in hc.G1_CASES} == set(range(1, 131)) | {312, 640}
    assert {n for _, _, n, _ in hc.G1_CASES} == set(hc.G1_N)


def test_one_lane_list_reaches_the_spill_past_the_first_piece():
    """d0 = A - V0 > 60 on the 64-byte grid (the initial register's bytes reach
    the second piece) in each burst size: records of <= 64, <= 128 and more bytes."""
    seen = set()
    for stride, L, n, r in hc.G1_CASES:
        for i in range(min(n, 4)):
            A = BASE + r + i * stride
            E = (A + L) & ~3                      # these walks grid records of < 8 bytes too
            V0 = E - (E - A + 63) // 64 * 64
            if L >= 8:
                assert (E, V0) == hc.step_geom(A, L, 64)[::2]
            if E > A and A - V0 > 60:
                seen.add(1 if L <= 64 else 2 if L <= 128 else 5)
    assert seen == {1, 2, 5}
    assert {(s - L) for s, L, _, _ in hc.G1_CASES} == {0, 1, 2, 3}


def test_multi_and_span_lists():
    for k in hc.MULTI_K:
        assert all(r % 16 == 0 for r in hc.multi_residues(k, 0))
        own = hc.multi_residues(k, 1)
        assert len(set(own)) == k and (k == 1 or any(r % 16 for r in own))
    assert set(hc.multi_residues(64, 1)) == set(hc.ALL64)
    assert min(hc.SPANS8_LENS) >= 16384 and len(hc.SPANS8_LENS) == len(hc.SPANS8_MIXED) == 8
    seen = set()
    for rot in range(8):
        rs = hc.spans8_residues(rot)
        assert len(set(rs)) == 8
        seen |= set(rs)
    assert {r % 4 for r in seen} == {0, 1, 2, 3} and len(seen) >= 15
    for bounded in (True, False):
        lens = hc.batch_lens(bounded)
        assert len(lens) == hc.BATCH_N and lens[0] > 0 and set(range(17)) <= set(lens)
        assert (max(lens) <= hc.BATCH_BOUND) == bounded
    assert max(hc.batch_lens(False)) > 1 << 20


def test_the_two_oracles_agree_and_seeds_combine():
    """crc32c_hw (the SSE4.2 instruction) against crc32c_py (the table walk in
    Python) on lengths up to 2048 at every alignment; and the identities the
    GPU tests derive seeded and raw expectations from."""
    rng = np.random.default_rng(2050)
    buf = rng.integers(0, 256, 2048 + 64, dtype=np.uint8)
    lens = sorted(set(range(0, 140)) | {312, 640, 700, 1021, 1024, 1037, 2047, 2048})
    for i, L in enumerate(lens):
        for off in (0, 1 + i % 3, 15 + i % 7):
            d = buf[off:off + L]
            for seed in (0, hc.SEED):
                assert oracle.crc32c_hw(seed, d) == oracle.crc32c_py(seed, d.tobytes()), (L, off, seed)
            c0 = oracle.crc32c_hw(0, d)
            assert oracle.crc32c_hw(hc.SEED, d) == oracle.shift(hc.SEED, L) ^ c0
            assert oracle.crc32c_hw(~hc.RAW_REG & 0xFFFFFFFF, d) == oracle.shift(~hc.RAW_REG & 0xFFFFFFFF, L) ^ c0
