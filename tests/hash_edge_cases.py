"""The shapes and base-address residues of tests/test_gpu_hash_edges.py, as
data, with the two geometry formulas of zscrc_kernels.hip restated in plain
Python so that tests/test_hash_edge_cases.py (CPU) can check that the lists
reach the branches they were chosen for.  No torch, no GPU.

A residue is the base address mod 64.  A case list pairs every length with
every residue it names; record counts and strides cycle over their sets along
the list, so each combination appears without the full cross product."""

SEED = 0xA5C31F27      # every byte non-zero: a register byte that spills into the next step is seen
RAW_REG = 0x5E17B3C9   # the raw calls' initial register, likewise

ALL64 = tuple(range(64))
# each phase (residue & 3) at a low, a middle and a high place in the 64-byte line
RESIDUES = (0, 1, 2, 3, 15, 16, 21, 34, 48, 49, 50, 63)


def qteam_geom(residue, length):
    """(ph, span, S, pad, tail) as qgeom(): the record's 4-byte phase, its
    bytes up to its last 4-aligned address, their 1 KiB steps, the grid's bytes
    before the record and the bytes after span."""
    ph = residue & 3
    span = ((ph + length) & ~3) - ph
    S = (span + 1023) // 1024
    return ph, span, S, S * 1024 - span, length - span


def step_geom(A, length, STEP):
    """(E, S, V0, tail) as team_kernel (STEP = G * 64), xteam_kernel (4096) and
    the one-lane walks (64) lay a record at address A on its step grid."""
    E = A if length < 8 else (A + length) & ~3
    S = 0 if length < 8 else (E - A + STEP - 1) // STEP
    return E, S, E - S * STEP, length - (E - A)


def _cycle(seq, i):
    return seq[i % len(seq)]


# ---- qteam_kernel / qteam_dyn_kernel (+qfold_kernel): n at the floor of the 16-lane rule
QTEAM_N = (16384, 16385, 16387)
QTEAM_LENS = tuple(2048 + d for d in range(9)) + tuple(3072 - d for d in range(9))
QTEAM_SHAPES = tuple((((L + 3) & ~3) + _cycle((0, 4, 64), i // 3), L, _cycle(QTEAM_N, i))
                     for i, L in enumerate(QTEAM_LENS)) + ((8200, 8195, 16385), (3000, 2050, 16387))
QTEAM_CASES = tuple((stride, L, n, r) for stride, L, n in QTEAM_SHAPES for r in RESIDUES)

# ---- team_kernel<16>: flattened walks (<= 2048, <= 8191), the two-level walk, odd strides
TEAM16_SHAPES = ((704, 700, 16385), (1039, 1037, 16384), (2048, 2048, 16387), (2051, 2049, 16384),
                 (4101, 4097, 16385), (8191, 8191, 16384), (8192, 8192, 16385), (8197, 8195, 16384),
                 (8264, 8200, 16387))

# ---- xteam_kernel and team_kernel<64>: steps of 4096 bytes, results stored 64 at a time
XSTEP = 4096
XTEAM_N = (1, 3, 63, 64, 65, 129)
XTEAM_LEN_GROUPS = (tuple(range(1, 17)), (63, 64, 65), tuple(range(4089, 4104)), tuple(range(8189, 8201)))


def xteam_cases(lens):
    """(stride, len, n, residue): every residue 0..63 at every length."""
    out = []
    for li, L in enumerate(lens):
        for r in ALL64:
            i = r + 64 * li
            out.append((L + (i // 6) % 2, L, _cycle(XTEAM_N, i), r))
    return tuple(out)


XTEAM_CASES = tuple(c for g in XTEAM_LEN_GROUPS for c in xteam_cases(g))


def spread8(L):
    """Eight residues for length L: each phase twice; all 64 over any 64 consecutive lengths."""
    return tuple((5 * L + 9 * k) % 64 for k in range(8))


# ---- team_kernel<2>
TEAM2_LENS = tuple(range(1, 301))
TEAM2_CASES = tuple((L + k % 2, L, _cycle(XTEAM_N, L + k), r)
                    for L in TEAM2_LENS for k, r in enumerate(spread8(L)))

# ---- one lane per record: team_kernel<1> rings, short_kernel, burst_kernel
G1_WALKS = (-1, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10)
G1_LENS = tuple(range(1, 131)) + (312, 640)
G1_N = (1, 63, 64, 65, 1000)
G1_CASES = tuple((L + (L + k) % 4, L, _cycle(G1_N, L + k), r)
                 for L in G1_LENS for k, r in enumerate(spread8(L)))

# ---- zscrc_device_fixed_multi: (stride, len), batches, records, zscrc_set_opt bits
MULTI_SHAPES = ((48, 40), (13, 11), (7, 5), (64, 64))
MULTI_K = (1, 3, 64)
MULTI_N = (1, 127, 129, 4099)
MULTI_OPTS = (0, 2, 1 << 21, 1 << 23)


def multi_residues(k, plan):
    """The residue of each of k bases: plan 0 all 16-byte aligned (what
    multi64_kernel wants of 64-byte records), plan 1 each base its own."""
    return tuple((16 * b) % 64 if plan == 0 else (7 * b + 3 * k) % 64 for b in range(k))


# ---- spans
SPAN_LENS = (0, 5, 16383, 16384, 16387, 65539, (1 << 20) + 5)
SPANS8_LENS = (16384, 16387, 65539, (1 << 20) + 5, 16385, 20000, 17407, 70001)   # all on the one-launch form
SPANS8_MIXED = (0, 5, 16383, 16384, 16387, 65539, 1, 70001)                      # short ones: a call each


def spans8_residues(rot):
    return tuple((9 * i + 9 * rot + 1) % 64 for i in range(8))


# ---- zscrc_device_batch_bounded: record lengths; the first record starts at the base
BATCH_N = 300
BATCH_BOUND = 600


def batch_lens(bounded):
    """BATCH_N lengths: tiny ones first (0..16 twice), then short ones up to
    the bound; unbounded, a few 16-lane and whole-wave records cut into parts
    (fewer of them than teams) among them."""
    lens = [5] + list(range(17)) * 2 + [(37 * i) % (BATCH_BOUND + 1) for i in range(BATCH_N - 35)]
    if not bounded:
        for at, L in ((40, 700), (90, 5000), (91, 8191), (150, 8192), (151, 20000), (220, 70001),
                      (221, 300001), (299, (1 << 20) + 7)):
            lens[at] = L
    assert len(lens) == BATCH_N
    return tuple(lens)
