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


@pytest.mark.parametrize("modulus", [4, 16, 64, 128, 512])
def test_dev_at_puts_the_bytes_at_the_residue_inside_junk(modulus):
    host = np.arange(1, 301, dtype=np.uint16).view(np.uint8)        # zeros among the data are kept
    for residue in sorted({0, 1, 3, modulus // 2 + 1, modulus - 1}):
        whole, view = dm.dev_at(host, CPU, residue, modulus)
        assert view.data_ptr() % modulus == residue and view.dtype == torch.uint8
        assert view.numpy().tobytes() == host.tobytes()
        before, after = dm.margins(whole, view)
        assert len(before) >= 4096 and len(after) >= 4096
        assert len(before) + len(after) + host.size == whole.numel()
        assert before.min() >= 1 and after.min() >= 1               # a missing mask reads no lucky zero
        assert len(set(before[-64:].tolist())) > 16                 # and no constant either
        view[0] = 0
        view[-1] = 0                                                # writes inside leave the margins alone
        b2, a2 = dm.margins(whole, view)
        assert np.array_equal(b2, before) and np.array_equal(a2, after)


def test_dev_at_margin_and_empty():
    whole, view = dm.dev_at(np.zeros(5, np.uint8), CPU, 7, 16, margin=100)
    before, after = dm.margins(whole, view)
    assert view.data_ptr() % 16 == 7 and len(before) >= 100 and len(after) >= 100
    assert before.min() >= 1 and after.min() >= 1 and not view.numpy().any()
    whole, view = dm.dev_at(np.zeros(0, np.uint8), CPU, 3)
    assert view.numel() == 0 and whole.cpu().numpy().min() >= 1
    with pytest.raises(AssertionError):
        dm.dev_at(np.zeros(5, np.uint8), CPU, 16, 16)


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


def test_fenced_many_sees_a_write_between_two_slices():
    n, k = 12, 3
    whole, outs = dm.fenced_many(n, k, CPU)
    assert whole.numel() == k * (n + dm.PAD) + dm.PAD and [o.numel() for o in outs] == [n] * k
    assert all(o.storage_offset() % 4 == 0 for o in outs)
    outs[1][:] = 7
    got = dm.inside_many(whole, n, k, "fine")
    assert [g.tolist() for g in got] == [[dm.CANARY] * n, [7] * n, [dm.CANARY] * n]
    for at in (0, outs[0].storage_offset() + n, outs[2].storage_offset() - 1, whole.numel() - 1):
        w2, _ = dm.fenced_many(n, k, CPU)
        w2[at] = 0
        with pytest.raises(AssertionError, match="case-%d" % at):
            dm.inside_many(w2, n, k, "case-%d" % at)


def test_all_canary():
    a, b = np.full(33, dm.CANARY, np.uint8), np.full(7, dm.CANARY, np.uint8)
    assert dm.all_canary(a, b) and dm.all_canary()
    b[6] ^= 1
    assert not dm.all_canary(a, b) and dm.all_canary(a, b[:6])
