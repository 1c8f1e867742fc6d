"""The conditions that keep the device-walk tests honest, from the host walk
alone (no GPU): the crafted boundary images build at production geometries,
the production-scale fuzz set holds every outcome in every default block, the
dense image overflows zscrc_device_verify_image's first walk, and the image
beyond 4 GiB is what tests/test_gpu_walk_scale.py takes it for."""
import numpy as np
import pytest

from tests import walk_images as wi
from tests.images import build_active
from zeroskip_amd import zsfile


@pytest.mark.parametrize("B,T", [(8192, 1024), (65536, 4096), (1 << 20, 16384)])
def test_boundary_cases_build(B, T):
    cases = wi.boundary_cases(B, T)  # its own asserts: every case is what its name says
    names = [n for n, _ in cases]
    assert len(set(names)) == len(names) == 15
    for name, img in cases:
        off, ln, rc, end = wi.host_walk(img)
        if name == "final_mid_file":
            assert rc == zsfile.STOPPED
        elif name.startswith("size_4") and name != "size_40":
            assert rc == zsfile.TRUNCATED
        else:
            assert (rc, end) == (zsfile.END, len(img)), name
        if not name.startswith("size_") and name != "final_mid_file":
            assert len(off) >= 1, name
    big = dict(cases)
    assert len(big["value_longer_than_two_blocks"]) > 2 * B
    assert len(big["ends_on_block_boundary"]) == B


def test_big_image_fills_three_default_blocks():
    img = wi.big_image()
    off, ln, rc, end = wi.host_walk(img)
    assert (rc, end) == (zsfile.END, len(img))
    at = off + ln  # the commit records' offsets
    for b in range(3):
        inside = int(((at >> 20) == b).sum())
        print(f"default block {b}: {inside} commits")
        assert inside >= 1000
    # small records throughout: no span is long enough to skip a default tile
    assert int(ln.max()) < 512


def test_big_fuzz_shares_and_spread():
    rcs = []
    stops = [0, 0, 0]
    for m in wi.big_fuzz():
        _, _, rc, end = wi.host_walk(m)
        rcs.append(rc)
        if rc != zsfile.END:
            assert end < 3 * wi.DEF_BLOCK
            stops[end // wi.DEF_BLOCK] += 1
    assert len(rcs) == wi.FUZZ_COUNT == 120
    for rc in (zsfile.END, zsfile.STOPPED, zsfile.TRUNCATED):
        share = rcs.count(rc) / len(rcs)
        print(f"host walk result {rc}: {share:.3f} of {len(rcs)} images")
        assert share >= 0.10, (rc, share)
    print("walks not ending at END, by default block of their end offset:", stops)
    assert min(stops) >= 5, stops


def test_dense_commit_image():
    img = wi.dense_commit_image(1000)  # asserts both facts itself
    assert len(img) == 40040 and len(img) > wi.DEF_TILE
    off, ln, rc, end = wi.host_walk(img)
    assert len(off) == 1000 > len(img) // 64 + 1 == 626
    assert (ln == 32).all()


@pytest.mark.parametrize("ntx,seed", [(200, 11), (30, 2)])
def test_unaligned_tail_image(ntx, seed):
    """The prefixes the GPU tests give it (tests/test_gpu_walk.py's wellformed,
    tests/test_gpu_walk_multi.py's image): the tail holds the image's shortest
    and its longest span, so res[3] / res[4] come from the one-lane walk."""
    prefix = build_active(ntx, seed=seed)
    poff, pln, _, _ = wi.host_walk(prefix)
    img, first, before = wi.unaligned_tail_image(prefix)
    off, ln, rc, end = wi.host_walk(img)
    assert (rc, end) == (zsfile.END, len(img)) and end % 8 == 4
    assert before == len(poff) == ntx and len(off) == before + 4
    assert first == len(prefix) + 52 and first % 8 == 4
    # build_active writes no transaction of 3 bytes or less, and none as long as the prefix
    assert int(ln.min()) == 3 and int(pln.min()) > 3
    assert int(ln.max()) == len(prefix) and int(pln.max()) < len(prefix)
    assert [int(v) for v in ln[before:]] == [12, 3, len(prefix), 20]


def test_huge_image_host_walk():
    pieces, size = wi.huge_image_pieces()
    assert size > (4 << 30) + (5 << 20)
    a = np.zeros(size, np.uint8)  # untouched pages are never backed by memory
    for at, b in pieces:
        a[at:at + len(b)] = np.frombuffer(b, np.uint8)
    n = wi.huge_commits()
    off, ln, rc, end = wi.host_walk_capped(a, n + 8)
    assert (rc, end, len(off)) == (zsfile.END, size, n)
    assert int(ln.max()) > 1 << 32 and int(off[-2]) == 40 and int(off[-2] + ln[-2]) > 1 << 32
    assert int(off[0]) > 1 << 32  # every span but the long commit's lies beyond 4 GiB
