"""What the zsdb_consistent tests share (tests/test_consistent_host.py on the
CPU, tests/test_gpu_consistent.py and tests/test_gpu_threads.py on the GPU): a
small DB written by the oracle's writer, its file names, and a stand-in for the
device passes computed with the CPU oracle.  No GPU is needed."""
import numpy as np
import torch

from oracle import oracle
from oracle import zs_format as zf
from tests.images import UUID, UUIDSTR

M32 = 0xFFFFFFFF


class OracleBackend:
    """Stand-in for the device passes, computed with the CPU oracle."""

    def empty(self, n):
        return torch.zeros(max(n, 1), dtype=torch.uint8)

    def verify(self, buf, off, ln, seed=None, max_len=None):
        # the bound the product passes to zscrc_device_verify_commits_bounded must hold
        assert max_len is None or all(n <= max_len for n in ln.tolist())
        img = buf.numpy()
        crc, st = [], []
        seeds = [0] * len(off) if seed is None else [v & M32 for v in seed.tolist()]
        for o, n, sd in zip(off.tolist(), ln.tolist(), seeds):
            try:
                _, _, _, stored, computed = zf._commit_check(img, o + n, sd)
                crc.append(computed)
                st.append(1 if stored == computed else 0)
            except ValueError:
                crc.append(0)
                st.append(2)
        as_i32 = lambda v: torch.tensor(np.array(v, np.uint32).view(np.int32))  # noqa: E731
        return as_i32(crc), as_i32(st)

    def raw(self, buf, off, ln):
        img = buf.numpy()
        r = [oracle.crc32c_hw(M32, img[o:o + n]) ^ M32 for o, n in zip(off.tolist(), ln.tolist())]
        return torch.tensor(np.array(r, np.uint32).view(np.int32))

    def crc(self, buf, off, ln, max_len=None):
        assert max_len is None or all(n <= max_len for n in ln.tolist())
        img = buf.numpy()
        r = [oracle.crc32c_hw(0, img[o:o + n]) for o, n in zip(off.tolist(), ln.tolist())]
        return torch.tensor(np.array(r, np.uint32).view(np.int32))

    def sync(self):
        pass


def name(*ix):
    return "zeroskip-" + UUIDSTR + "".join(f"-{i}" for i in ix)


def small_db(long_region: bool = False, seed: int = 7) -> dict:
    """packed(0-3) [+ long packed(4-5)], finalised 6..8 (with the finalise
    quirk), active 9, .zsdb -- every CRC from the oracle writer."""
    rng = np.random.default_rng(seed)
    db = {}
    recs = [(b"k%05d" % i, rng.integers(0, 256, int(rng.integers(0, 300)), dtype=np.uint8).tobytes())
            for i in range(400)]
    db[name(0, 3)] = zf.packed_file(recs, UUID, 0, 3)
    idx = 4
    if long_region:
        big = [(b"b%05d" % i, rng.integers(0, 256, 70000, dtype=np.uint8).tobytes()) for i in range(250)]
        db[name(4, 5)] = zf.packed_file(big, UUID, 4, 5)
        idx = 6
    for f in range(3):
        w = zf.FileWriter(UUID, idx)
        for t in range(40):
            for j in range(int(rng.integers(1, 4))):
                w.add(b"f%d-%d-%d" % (f, t, j), rng.integers(0, 256, int(rng.integers(0, 500)), dtype=np.uint8).tobytes())
            if t % 7 == 3:
                w.remove(b"f%d-%d-0" % (f, t))
            w.commit()
        w.finalise()
        db[name(idx, idx)] = w.image()
        idx += 1
    w = zf.FileWriter(UUID, idx)
    for t in range(10):
        w.add(b"a%d" % t, b"v" * t)
        w.commit()
    db[name(idx)] = w.image()
    db[".zsdb"] = zf.dotzsdb_bytes(len(db[name(idx)]), UUIDSTR.encode() + b"\0", idx)
    return db
