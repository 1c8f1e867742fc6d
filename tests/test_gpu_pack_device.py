"""The device packer (zscrc_device_pack, zeroskip_amd/csrc/zscrc_devpack.hip)
against the host packer (repack.Packer) on the same records, byte for byte, and
against the format oracle where it accepts the list.  Output buffers are
canary-filled between fences: bytes at and after file_bytes and the fences must
still hold the canary.  The record lists are tests/pack_cases.py's."""
import numpy as np
import pytest
import torch

from oracle import zs_format as zf
from tests import devmem as dm
from tests import pack_cases as pc
from tests import records_images as ri
from tests.devmem import CANARY
from tests.images import EINVAL64, OVERFLOW, U64_MAX
from zeroskip_amd import repack, zsfile

pytestmark = pytest.mark.gpu

TILES = [64, 128, 4096, 0]
TILE_IDS = ["t64", "t128", "t4096", "default"]


def _bound(recs: np.ndarray) -> int:
    """zscrc_device_pack_bound from what the lister's res[1], res[4], res[5] hold for the list."""
    with np.errstate(over="ignore"):
        return repack.device_pack_bound(len(recs), int(recs[:, 1].sum(dtype=np.uint64)),
                                        int(recs[:, 3].sum(dtype=np.uint64)))


def _pack(d_src, d_recs, case, cap, tile=0, scratch=None):
    """device_pack into `cap` canary bytes between fences: (the cap bytes, res uint64[8])."""
    dev = d_src.device
    whole, out = dm.fenced(cap, dev)
    assert out.data_ptr() % 16 == 0
    _, res = repack.device_pack(d_src, d_recs, case.uuid, case.startidx, case.endidx, out=out, tile_bytes=tile,
                                scratch=scratch)
    r = res.cpu().numpy().view(np.uint64)
    return dm.inside(whole, cap, case.name), r


def _same(case, dev, want: bytes, tile=0, shift=0, slack=64, d_recs=None, d_src=None, scratch=None):
    """The case packed into len(want) + slack bytes equals want; returns res."""
    d_src = dm.dev_bytes(case.src, dev, shift) if d_src is None else d_src
    d_recs = dm.dev_recs(case.recs, dev) if d_recs is None else d_recs
    got, r = _pack(d_src, d_recs, case, len(want) + slack, tile, scratch)
    what = (case.name, tile, shift)
    assert [int(v) for v in r[:3]] == [0, len(case.recs), len(want)], (what, r)
    assert got[:len(want)].tobytes() == want, what
    assert bool((got[len(want):] == CANARY).all()), what      # nothing at or after file_bytes
    assert _bound(case.recs) >= len(want), what
    return r


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in pc.small_cases()}


@pytest.fixture(scope="module")
def host_files(gpu, cases, tmp_path_factory):
    """The host packer's file and report for every small case, written once."""
    d = tmp_path_factory.mktemp("host_packer")
    out = {}
    for i, c in enumerate(cases.values()):
        rep, img = pc.host_packer_file(c, d / ("f%d" % i))
        assert img == c.want, c.name                          # the oracle (or the source file) agrees
        out[c.name] = (rep, img)
    return out


# ------------------------------------------------------------- empty and single
def test_empty_and_single(gpu, cases, host_files):
    r = _same(cases["empty"], gpu, host_files["empty"][1])
    assert int(r[2]) == 64 and int(r[3]) == 0
    for tile in (64, 0):
        for name in ("empty", "single_kv", "single_delete", "empty_key_and_value"):
            _same(cases[name], gpu, host_files[name][1], tile=tile)


# --------------------------------------------------------------- alignment grid
@pytest.mark.parametrize("tile", TILES, ids=TILE_IDS)
def test_alignment_grid(gpu, cases, host_files, tile):
    c = cases["alignment_grid"]
    d_recs = dm.dev_recs(c.recs, gpu)
    for shift in range(8):
        _same(c, gpu, host_files[c.name][1], tile=tile, shift=shift, d_recs=d_recs)


# -------------------------------------------------------------- tile boundaries
def test_tile_boundaries(gpu, cases, host_files):
    for name in ("tile_boundaries", "region_64", "region_56", "region_72", "region_24", "region_128_two_records"):
        for tile in (64, 128, 16384):
            _same(cases[name], gpu, host_files[name][1], tile=tile)
    _same(cases["tile_boundaries"], gpu, host_files["tile_boundaries"][1], shift=3)


# -------------------------------------------------------------------- log order
def test_log_order_without_leaving_the_device(gpu, cases, host_files):
    c = cases["log_order"]
    d = dm.dev_bytes(c.src, gpu)
    recs, res = zsfile.device_records(d, zsfile.ACTIVE)
    lr = res.cpu().numpy().view(np.uint64)
    n = int(lr[1])
    assert int(lr[0]) == zsfile.END and n == len(c.recs)
    want = host_files[c.name][1]
    assert repack.device_pack_bound(n, int(lr[4]), int(lr[5])) >= len(want)
    for tile in (64, 0):
        _same(c, gpu, want, tile=tile, d_src=d, d_recs=recs[:n])
    img, res = repack.device_pack(d, recs[:n], c.uuid, c.startidx, c.endidx)     # out=None: sized by the wrapper
    assert img.numel() == len(want) and img.cpu().numpy().tobytes() == want


# ------------------------------------------------------------------ round trips
def test_round_trips(gpu, cases, host_files):
    names = [n for n in cases if n.startswith(("packed_small", "golden_"))]
    assert len(names) == 5
    for name in names:
        c = cases[name]
        d = dm.dev_bytes(c.src, gpu)
        recs, res = zsfile.device_records(d, zsfile.PACKED)
        lr = res.cpu().numpy().view(np.uint64)
        n = int(lr[1])
        assert int(lr[0]) == 0 and n == len(c.recs)
        assert repack.device_pack_bound(n, int(lr[4]), int(lr[5])) >= len(c.src)
        for tile in (64, 0):
            _same(c, gpu, c.src, tile=tile, d_src=d, d_recs=recs[:n])            # input == output
        assert host_files[name][1] == c.src


def test_regenerated_headers(gpu, cases, host_files):
    c = cases["regenerated_headers"]
    assert c.want != c.src and c.want == zf.packed_file(c.pairs(), c.uuid, c.startidx, c.endidx)
    for tile in (64, 0):
        _same(c, gpu, c.want, tile=tile)


# ------------------------------------------------------------------- long forms
def test_long_commit_long_records(gpu, tmp_path):
    """Long value, long key and long records-region commit in one file of about 40 MB."""
    c, pairs = pc.long_commit_long_records()
    rep, want = pc.host_packer_file(c, tmp_path / "h")
    assert want == zf.packed_file(pairs, c.uuid, c.startidx, c.endidx) and rep["region_bytes"] > zf.MAX_SHORT_VAL_LEN
    r = _same(c, gpu, want)
    assert [int(v) for v in r[3:8]] == [rep["region_bytes"], rep["region_crc"], rep["pointers_crc"],
                                        rep["commit_crc"], rep["final_crc"]]
    _same(c, gpu, want, tile=65536, shift=5)


def test_long_final_commit(gpu, tmp_path):
    """2,097,152 deletes of one shared 1-byte key: a pointer section above
    16,777,215 bytes (long final commit), a 50 MB region."""
    n = 2097152
    recs = np.zeros((n, 4), np.uint64)
    recs[:, 0], recs[:, 1], recs[:, 2] = 3, 1, U64_MAX
    c = pc.Case("long_final_commit", b"abcKdef", recs, want=b"")
    rep, want = pc.host_packer_file(c, tmp_path / "h")
    assert 8 * (n + 1) > zf.MAX_SHORT_VAL_LEN and want[-24] == zf.REC_LONG_FINAL and len(want) == 40 + 32 * n + 24 + 8 * (n + 1) + 24
    r = _same(c, gpu, want)
    assert [int(v) for v in r[3:8]] == [rep["region_bytes"], rep["region_crc"], rep["pointers_crc"],
                                        rep["commit_crc"], rep["final_crc"]]


def test_long_delete(gpu, cases, host_files):
    c = cases["long_delete"]
    want = host_files[c.name][1]                              # the host packer's file only: the oracle refuses it
    at = 40 + len(zf.key_record(b"a") + zf.value_record(b"1"))
    assert want[at:at + 24] == zf.be64(0) + zf.be64(70000) + zf.be64(0)
    for tile in (64, 0):
        _same(c, gpu, want, tile=tile, shift=1)


def test_shared_and_overlapping_source_bytes(gpu, cases, host_files):
    c = cases["shared_bytes"]
    for tile in (64, 0):
        _same(c, gpu, host_files[c.name][1], tile=tile)


# --------------------------------------------------------------------- capacity
def test_capacity(gpu, cases, host_files):
    for name in ("log_order", "single_kv", "empty"):
        c, want = cases[name], host_files[name][1]
        region = host_files[name][0]["region_bytes"]
        d_src, d_recs = dm.dev_bytes(c.src, gpu), dm.dev_recs(c.recs, gpu)
        _same(c, gpu, want, slack=0, d_src=d_src, d_recs=d_recs)          # out_cap == file_bytes
        for cap in (len(want) - 1, len(want) - 16, 48, 0):
            got, r = _pack(d_src, d_recs, c, cap)
            assert [int(v) for v in r] == [OVERFLOW, len(c.recs), len(want), region, 0, 0, 0, 0], (name, cap, r)
            assert bool((got == CANARY).all()), (name, cap)
        # the sizing call: no output at all
        res = torch.empty(repack.PACK_RES_WORDS, dtype=torch.int64, device=gpu)
        out, res = repack.device_pack(d_src, d_recs, c.uuid, c.startidx, c.endidx,
                                      out=torch.empty(0, dtype=torch.uint8, device=gpu))
        assert [int(v) for v in res.cpu().numpy()[:4]] == [OVERFLOW, len(c.recs), len(want), region]


# ------------------------------------------------------------------ bad records
def test_bad_records(gpu, cases, host_files):
    c = cases["log_order"]
    n, size = len(c.recs), len(c.src)
    d_src = dm.dev_bytes(c.src, gpu)
    live = int(np.flatnonzero(c.recs[:, 2] != U64_MAX)[5])

    def bad(changes, first):
        recs = c.recs.copy()
        for i, col, v in changes:
            recs[i, col] = v
        got, r = _pack(d_src, dm.dev_recs(recs, gpu), c, len(c.want) + 64, tile=64)
        assert int(r[0]) == EINVAL64 and int(r[1]) == first, (changes, r)
        assert [int(v) for v in r[4:8]] == [0, 0, 0, 0]
        assert bool((got == CANARY).all()), changes

    k = int(c.recs[9, 1])
    bad([(9, 0, size - k + 1)], 9)                                   # key end one byte past src_size
    bad([(live, 2, size - 3), (live, 3, 40)], live)                  # value end past src_size
    bad([(n - 1, 0, U64_MAX - 3), (n - 1, 1, 8)], n - 1)             # key_off = 2^64 - 4 with length 8
    bad([(0, 1, U64_MAX)], 0)                                        # key_len = 2^64 - 1
    bad([(live, 2, U64_MAX - 1)], live)                              # a value offset that is almost DELETED
    bad([(n - 2, 1, U64_MAX), (1500 % n, 0, size + 1), (live, 3, size + 1), (n // 2, 0, U64_MAX - 3)],
        min(n - 2, 1500 % n, live, n // 2))                          # several at once: the smallest index
    # at the edge and legal: a key that ends exactly at src_size, an empty key at src_size
    recs = c.recs.copy()
    recs[3] = (size - 5, 5, size, 0)
    recs[4] = (size, 0, U64_MAX, 0)
    got, r = _pack(d_src, dm.dev_recs(recs, gpu), c, len(c.want) + 4096, tile=64)
    ok = pc.Case("edge", c.src, recs)
    assert int(r[0]) == 0 and got[:int(r[2])].tobytes() == ok.want


# ------------------------------------------------------ result and verification
def test_result_words_and_verification(gpu, cases, host_files):
    for name in ("log_order", "alignment_grid", "empty", "long_delete"):
        c = cases[name]
        rep, want = host_files[name]
        r = _same(c, gpu, want)
        assert [int(v) for v in r] == [0, rep["records"], rep["file_bytes"], rep["region_bytes"], rep["region_crc"],
                                       rep["pointers_crc"], rep["commit_crc"], rep["final_crc"]], name
    c = cases["log_order"]
    img, _ = repack.device_pack(dm.dev_bytes(c.src, gpu), dm.dev_recs(c.recs, gpu), c.uuid, c.startidx, c.endidx)
    v = zsfile.verify_device_image(img, zsfile.PACKED)
    assert v["walk_rc"] == 0 and v["n_commits"] == 2 and v["n_bad"] == 0 and v["header_rc"] == 0
    assert v["header_stored"] == v["header_computed"]
    recs, res = zsfile.device_records(img, zsfile.PACKED)
    lr = res.cpu().numpy().view(np.uint64)
    assert int(lr[0]) == 0 and int(lr[1]) == len(c.recs)
    packed = img.cpu().numpy().tobytes()
    assert ri.as_pairs(packed, recs[:len(c.recs)].cpu().numpy().view(np.uint64)) == c.pairs()


# ------------------------------------------- scratch, streams and determinism
def test_caller_scratch_fenced(gpu, cases, host_files):
    for name, tile in (("log_order", 0), ("alignment_grid", 64), ("empty", 0)):
        c = cases[name]
        need = repack.device_pack_scratch_bytes(len(c.recs), tile)
        assert need > 0
        whole, scratch = dm.fenced(need, gpu)
        assert scratch.data_ptr() % 16 == 0
        _same(c, gpu, host_files[name][1], tile=tile, scratch=scratch)
        assert dm.intact(whole, need), name


def test_library_scratch_from_two_streams(gpu, cases, host_files):
    """Two packs on two streams share the library's scratch, ordered by its event."""
    a, b = cases["log_order"], cases["alignment_grid"]
    sa, ra, sb, rb = dm.dev_bytes(a.src, gpu), dm.dev_recs(a.recs, gpu), dm.dev_bytes(b.src, gpu), dm.dev_recs(b.recs, gpu)
    wa, oa = dm.fenced(len(a.want) + 64, gpu)
    wb, ob = dm.fenced(len(b.want) + 64, gpu)
    s1, s2 = torch.cuda.Stream(device=gpu), torch.cuda.Stream(device=gpu)
    torch.cuda.synchronize(gpu)
    results = []
    for _ in range(3):
        with torch.cuda.stream(s1):
            results.append((a, oa, repack.device_pack(sa, ra, a.uuid, a.startidx, a.endidx, out=oa)[1]))
        with torch.cuda.stream(s2):
            results.append((b, ob, repack.device_pack(sb, rb, b.uuid, b.startidx, b.endidx, out=ob, tile_bytes=128)[1]))
    torch.cuda.synchronize(gpu)
    for c, o, res in results:
        r = res.cpu().numpy().view(np.uint64)
        assert [int(v) for v in r[:3]] == [0, len(c.recs), len(c.want)], c.name
        assert o.cpu().numpy()[:len(c.want)].tobytes() == host_files[c.name][1], c.name


def test_side_stream(gpu, cases, host_files):
    c = cases["tile_boundaries"]
    side = torch.cuda.Stream(device=gpu)
    d_src, d_recs = dm.dev_bytes(c.src, gpu), dm.dev_recs(c.recs, gpu)
    torch.cuda.synchronize(gpu)
    with torch.cuda.stream(side):
        _same(c, gpu, host_files[c.name][1], tile=64, d_src=d_src, d_recs=d_recs)


def test_two_runs_bit_for_bit(gpu, cases):
    for name, tile in (("log_order", 0), ("alignment_grid", 64)):
        c = cases[name]
        d_src, d_recs = dm.dev_bytes(c.src, gpu), dm.dev_recs(c.recs, gpu)
        a = _pack(d_src, d_recs, c, len(c.want) + 64, tile)
        b = _pack(d_src, d_recs, c, len(c.want) + 64, tile)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
