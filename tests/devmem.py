"""What the device tests share: uploads at a chosen address residue, and output
buffers between two fences of canary bytes.  A kernel that writes outside its
output is seen by `intact` / `inside` only, so there is one copy of them.
Runs on any torch device (tests/test_devmem.py checks it on the CPU)."""
import numpy as np
import torch

CANARY = 0xA5
PAD = 4096      # canary bytes on each side of every fenced buffer


def dev_bytes(b: bytes, dev, shift: int = 0) -> torch.Tensor:
    """The bytes in device memory at an address = shift mod 16 (an empty tensor for none)."""
    buf = torch.zeros(len(b) + 32, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    d = buf[shift:shift + len(b)]
    if len(b):
        d.copy_(torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()))
    return d


def dev_recs(a: np.ndarray, dev) -> torch.Tensor:
    """A host list of 32-byte entries (records, queries, gather's items) as an int64 [n, 4] device tensor."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1, 4).copy()).to(dev)


def fenced(nbytes: int, dev):
    """(whole, out): nbytes of canary with PAD canary bytes on each side; out is the slice between them."""
    whole = torch.full((nbytes + 2 * PAD,), CANARY, dtype=torch.uint8, device=dev)
    return whole, whole[PAD:PAD + nbytes]


def intact(whole: torch.Tensor, nbytes: int) -> bool:
    """Both fences of fenced(nbytes, ...)'s whole still hold the canary."""
    h = whole.cpu().numpy()
    return bool((h[:PAD] == CANARY).all() and (h[PAD + nbytes:] == CANARY).all())


def inside(whole: torch.Tensor, nbytes: int, what=None) -> np.ndarray:
    """The host copy of the bytes between the fences, which must hold; `what`
    names the case in the failure (asserts here are not rewritten by pytest)."""
    h = whole.cpu().numpy()
    assert bool((h[:PAD] == CANARY).all() and (h[PAD + nbytes:] == CANARY).all()), what
    return h[PAD:PAD + nbytes]


def all_canary(*arrays) -> bool:
    return all(bool((a == CANARY).all()) for a in arrays)


def dev_in(case, dev, shift=0, qshift=0):
    """A find / scan / next case on the device: (src, [(records, base)], query bytes, queries)."""
    return (dev_bytes(case.src, dev, shift), [(dev_recs(r, dev), b) for r, b in case.levels],
            dev_bytes(case.qsrc, dev, qshift), dev_recs(case.queries, dev))
