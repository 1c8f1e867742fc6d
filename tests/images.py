"""The root of the tests' support modules: the constants every case module
shares and the small active image most image builders start from.  It imports
no other module of tests/; no GPU is needed."""
import os

import numpy as np

from oracle import zs_format as zf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "tests", "golden", "ref_format")     # the reference-written fixtures
UUID = bytes(range(16))
UUIDSTR = "00010203-0405-0607-0809-0a0b0c0d0e0f"              # UUID as the fixtures' file names spell it
U64_MAX = (1 << 64) - 1
EINVAL64 = U64_MAX  # (uint64_t)(int64_t)ZSCRC_EINVAL
OVERFLOW = 3        # ZSCRC_ZS_OVERFLOW


def build_active(ntx=50, seed=1):
    rng = np.random.default_rng(seed)
    w = zf.FileWriter(UUID, idx=3)
    for t in range(ntx):
        for _ in range(int(rng.integers(1, 4))):
            k = b"%016d" % int(rng.integers(0, 10**9))
            v = rng.integers(0, 256, int(rng.integers(0, 600)), dtype=np.uint8).tobytes()
            w.add(k, v)
        if t % 7 == 3:
            w.remove(b"%016d" % t)       # zeroskip.c:985 quirk: span restarts here
        w.commit()
    return w.image()


def zsbench_db(per_file, gaps, seed=5):
    """zsbench BATCHED-like files (one 16-byte key + 256-byte value per
    transaction: 312-byte spans every 320 bytes) concatenated with `gaps`
    bytes between them (shifts every file's piece grid)."""
    rng = np.random.default_rng(seed)
    parts, offs, lens, commits = [], [], [], []
    base = 0
    for f, (n, gap) in enumerate(zip(per_file, gaps)):
        parts.append(bytes(rng.integers(0, 256, gap, dtype=np.uint8)))
        base += gap
        w = zf.FileWriter(UUID, idx=f)
        for t in range(n):
            w.add(b"%016d" % (f * 100000 + t), rng.integers(0, 256, 256, dtype=np.uint8).tobytes())
            w.commit()
        if f % 2:
            w.finalise()              # a stale zero-length commit after the last span
        img = w.image()
        cs, _, _ = zf.walk(img)
        for c in cs:
            offs.append(base + c["span_off"])
            lens.append(c["span_len"])
            commits.append(c)
        parts.append(img)
        base += len(img)
    host = np.frombuffer(b"".join(parts), np.uint8).copy()
    return host, np.array(offs, np.int64), np.array(lens, np.int64), commits


def oracle_bad(img, offs, lens, cs_by_off, seeds=None):
    """indices whose commit does not verify (outside the image: no commit)"""
    hb = img.tobytes()
    want = set()
    for i, (o, n) in enumerate(zip(offs, lens)):
        o, n = int(o), int(n)
        if o > len(hb) or n > len(hb) - o or len(hb) - o - n < 8:
            want.add(i)
            continue
        try:
            _, _, _, stored, comp = zf._commit_check(hb, o + n, 0 if seeds is None else int(seeds[i]))
        except ValueError:
            want.add(i)
            continue
        if stored != comp:
            want.add(i)
    return want
