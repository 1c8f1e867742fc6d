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


def junk(n: int, seed: int) -> np.ndarray:
    """n seeded pseudo-random bytes in 1..255: what surrounds the data of dev_at."""
    return np.random.default_rng(seed).integers(1, 256, n, dtype=np.uint8)


def dev_at(host: np.ndarray, dev, residue: int, modulus: int = 64, margin: int = 4096):
    """(whole, view): the bytes of `host` in device memory at an address =
    residue mod modulus, inside one allocation whose every other byte -- at
    least `margin` on each side -- is junk() (never zero: a kernel that reads
    before or past the data and forgets to mask it gets a wrong value, not a
    fault and not a lucky zero).  The slice start comes from the allocation's
    own address, whatever its alignment."""
    assert 0 <= residue < modulus and margin > 0
    h = np.ascontiguousarray(host).view(np.uint8).reshape(-1)
    whole = torch.empty(h.size + 2 * margin + modulus, dtype=torch.uint8, device=dev)
    start = margin + (residue - whole.data_ptr() - margin) % modulus
    image = junk(whole.numel(), h.size * 31 + residue)
    image[start:start + h.size] = h
    whole.copy_(torch.from_numpy(image))
    view = whole[start:start + h.size]
    assert h.size == 0 or view.data_ptr() % modulus == residue
    return whole, view


def margins(whole: torch.Tensor, view: torch.Tensor):
    """The host copies of dev_at's bytes before and after the view."""
    start = view.storage_offset()
    h = whole.cpu().numpy()
    return h[:start], h[start + view.numel():]


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


def fenced_many(nbytes: int, k: int, dev):
    """(whole, outs): k slices of nbytes (a multiple of 4) in one canary
    buffer, PAD canary bytes before, between and after them."""
    assert nbytes % 4 == 0
    whole = torch.full((k * (nbytes + PAD) + PAD,), CANARY, dtype=torch.uint8, device=dev)
    return whole, [whole[PAD + i * (nbytes + PAD):PAD + i * (nbytes + PAD) + nbytes] for i in range(k)]


def inside_many(whole: torch.Tensor, nbytes: int, k: int, what=None) -> list:
    """The host copies of fenced_many's k slices; every byte around them must hold."""
    h = whole.cpu().numpy()
    outs = []
    for i in range(k + 1):
        at = i * (nbytes + PAD)
        assert bool((h[at:at + PAD] == CANARY).all()), (what, "fence", i)
        if i < k:
            outs.append(h[at + PAD:at + PAD + nbytes])
    return outs


def all_canary(*arrays) -> bool:
    return all(bool((a == CANARY).all()) for a in arrays)


def dev_in(case, dev, shift=0, qshift=0):
    """A find / scan / next case on the device: (src, [(records, base)], query bytes, queries)."""
    return (dev_bytes(case.src, dev, shift), [(dev_recs(r, dev), b) for r, b in case.levels],
            dev_bytes(case.qsrc, dev, qshift), dev_recs(case.queries, dev))
