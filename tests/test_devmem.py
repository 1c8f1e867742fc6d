"""tests/devmem.py, the uploads and the fence check the device tests share, on
torch's CPU device: a write outside a fenced slice is seen, one inside is not.
No GPU."""
import numpy as np
import pytest
import torch

from tests import devmem as dm

CPU = torch.device("cpu")


def test_dev_bytes_at_every_shift():
    b = bytes(range(1, 78))
    for shift in range(16):
        d = dm.dev_bytes(b, CPU, shift)
        assert d.data_ptr() % 16 == shift and d.dtype == torch.uint8
        assert d.numpy().tobytes() == b
        e = dm.dev_bytes(b"", CPU, shift)
        assert e.numel() == 0 and e.dtype == torch.uint8


def test_dev_recs_is_the_list_as_int64_rows():
    a = np.arange(12, dtype=np.uint64).reshape(3, 4)
    a[1, 2] = (1 << 64) - 1
    d = dm.dev_recs(a[::-1], CPU)                  # a view that is not contiguous
    assert d.dtype == torch.int64 and tuple(d.shape) == (3, 4)
    assert d.numpy().view(np.uint64).tolist() == a[::-1].tolist()
    assert tuple(dm.dev_recs(np.zeros((0, 4), np.uint64), CPU).shape) == (0, 4)


@pytest.mark.parametrize("n", [0, 1, 4096])
def test_a_write_outside_the_slice_is_seen(n):
    for at in (dm.PAD - 1, dm.PAD + n, n + 2 * dm.PAD - 1):
        whole, out = dm.fenced(n, CPU)
        assert whole.numel() == n + 2 * dm.PAD and out.numel() == n and out.storage_offset() == dm.PAD
        assert dm.intact(whole, n) and dm.inside(whole, n, "untouched").tobytes() == bytes([dm.CANARY]) * n
        whole[at] = 0
        assert not dm.intact(whole, n)
        with pytest.raises(AssertionError, match="case-%d-%d" % (n, at)):
            dm.inside(whole, n, "case-%d-%d" % (n, at))


@pytest.mark.parametrize("n", [1, 4096])
def test_a_write_inside_the_slice_is_not(n):
    for at in (0, n - 1):
        whole, out = dm.fenced(n, CPU)
        out[at] = 0
        assert dm.intact(whole, n)
        got = dm.inside(whole, n, "inside")
        assert len(got) == n and got[at] == 0 and int((got != dm.CANARY).sum()) == 1


def test_all_canary():
    a, b = np.full(33, dm.CANARY, np.uint8), np.full(7, dm.CANARY, np.uint8)
    assert dm.all_canary(a, b) and dm.all_canary()
    b[6] ^= 1
    assert not dm.all_canary(a, b) and dm.all_canary(a, b[:6])
