"""The device log writer (zscrc_device_log, zeroskip_amd/csrc/zscrc_devlog.hip)
against the format oracle's FileWriter, byte for byte, on the cases of
tests/log_cases.py, and against its host twin (zscrc_zs_log) for the result
words and the optional outputs.  Output buffers are canary-filled between
fences: the bytes before `at`, at and after the end offset and the fences must
still hold what they held.  Then the round trips through the stages that
already exist (lister, verifier, merge, packer), a seeded soak, and one call
whose offsets lie beyond 4 GiB."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import zs_format as zf
from tests import devmem as dm
from tests import log_cases as lc
from tests import pack_cases as pc
from tests import records_images as ri
from tests.devmem import CANARY
from tests.log_cases import check_against_image
from zeroskip_amd import repack, zsfile
from zeroskip_amd._lib import check, lib

pytestmark = pytest.mark.gpu

TILES = [64, 4096, 0]
TILE_IDS = ["t64", "t4096", "default"]
WORDS = ("code", "n", "end", "written", "commits", "long_commits", "last_crc", "stored_crc")


def _dev_tx(case, dev):
    return None if case.tx_end is None else torch.tensor(case.tx_end, dtype=torch.int64, device=dev)


def run_dev(case, dev, cap, tile=0, shift=0, scratch=None):
    """device_log of the case into `cap` canary bytes between fences, the prefix
    in place: (result dict with host copies, the cap bytes)."""
    whole, out = dm.fenced(cap, dev)
    assert out.data_ptr() % 16 == 0
    if case.at and cap >= case.at:
        out[:case.at].copy_(torch.from_numpy(np.frombuffer(case.prefix, np.uint8).copy()))
    d_src = out[:case.at] if case.src_in_prefix else dm.dev_bytes(case.src, dev, shift)
    d = zsfile.device_log(d_src, dm.dev_recs(case.recs, dev), _dev_tx(case, dev), case.uuid, case.startidx,
                          case.endidx, out=out, at=case.at, finalise=case.finalise, prev_crc=case.prev_crc,
                          tile_bytes=tile, new_recs=True, spans=True, scratch=scratch)
    got = dm.inside(whole, cap, case.name)
    for k in ("new_recs", "span_off", "span_len"):
        if d[k] is not None:
            d[k] = d[k].cpu().numpy().view(np.uint64)
    return d, got


def same(case, dev, tile=0, shift=0, slack=64, scratch=None):
    """The case written into len(want) + slack bytes equals the oracle's image and the host twin's words."""
    want = case.want
    d, got = run_dev(case, dev, len(want) + slack, tile, shift, scratch)
    what = (case.name, tile, shift)
    assert d["code"] == 0 and d["end"] == len(want), (what, [d[k] for k in WORDS])
    assert got[:len(want)].tobytes() == want, what
    assert bool((got[len(want):] == CANARY).all()), what          # nothing at or after the end offset
    h = host_result(case)
    assert [d[k] for k in WORDS] == [h[k] for k in WORDS], what
    for k in ("new_recs", "span_off", "span_len"):
        assert np.array_equal(d[k].reshape(-1), np.asarray(h[k]).view(np.uint64).reshape(-1)), (what, k)
    return d, got


_HOST = {}


def host_result(case):
    """The host twin's result for the case, computed once and checked against the oracle's image."""
    if case.name not in _HOST:
        out = np.full(len(case.want) + 64, CANARY, np.uint8)
        out[:case.at] = np.frombuffer(case.prefix, np.uint8)
        d = zsfile.log(case.src, case.recs, case.tx_end, case.uuid, case.startidx, case.endidx, out=out, at=case.at,
                       finalise=case.finalise, prev_crc=case.prev_crc, new_recs=True, spans=True)
        check_against_image(case, d, out.tobytes())
        _HOST[case.name] = d
    return _HOST[case.name]


# ------------------------------------------------------------------ the cases
@pytest.mark.parametrize("tile", TILES, ids=TILE_IDS)
def test_every_small_case(gpu, tile):
    cases = lc.small_cases()
    assert len(cases) >= 160
    for case in cases:
        same(case, gpu, tile=tile)


@pytest.mark.parametrize("tile", TILES, ids=TILE_IDS)
def test_source_alignments(gpu, tile):
    for case in lc.small_cases():
        if case.name in ("alignment_grid", "shared_bytes", "count_130"):
            for shift in range(1, 8):
                same(case, gpu, tile=tile, shift=shift)


@pytest.mark.parametrize("i", range(4))
def test_big_cases(gpu, i):
    """Values and spans around 16,777,215 bytes at the default tile; the long span of small records at 64 too."""
    case = lc.big_cases()[i]
    d, _ = same(case, gpu, slack=16)
    assert d["long_commits"] == (0 if case.name == "span_16777208" else 1)
    if case.name == "long_span_small_records":
        same(case, gpu, tile=64, shift=3, slack=16)


def test_exact_capacity_and_sized_by_the_wrapper(gpu):
    for case in lc.appends() + [c for c in lc.small_cases() if c.name in ("single_kv", "count_77", "empty_no_table")]:
        same(case, gpu, slack=0)                                          # out_cap == the end offset
        if case.at:
            continue
        d = zsfile.device_log(dm.dev_bytes(case.src, gpu), dm.dev_recs(case.recs, gpu), _dev_tx(case, gpu), case.uuid,
                              case.startidx, case.endidx, finalise=case.finalise)       # out=None
        assert d["code"] == 0 and d["image"].cpu().numpy().tobytes() == case.want, case.name


# ------------------------------------------------------------------ bad input
@pytest.mark.parametrize("tile", [64, 0], ids=["t64", "default"])
def test_bad_inputs_leave_everything_untouched(gpu, tile):
    base, bad = lc.bad_inputs()
    for name, case, cap, head in bad:
        cap = len(base.want) + 64 if cap is None else cap
        whole, out = dm.fenced(cap, gpu)
        nr = torch.full((case.n, 4), 0x5A5A, dtype=torch.int64, device=gpu)
        so = torch.full((8,), 0x5A5A, dtype=torch.int64, device=gpu)
        sl = torch.full((8,), 0x5A5A, dtype=torch.int64, device=gpu)
        res = torch.full((8,), 0x77, dtype=torch.int64, device=gpu)
        te = torch.tensor(case.tx_end, dtype=torch.int64, device=gpu)
        d_src, d_recs = dm.dev_bytes(case.src, gpu), dm.dev_recs(case.recs, gpu)
        opts = zsfile.LogOpts(tile, 0)
        check(lib().zscrc_device_log(d_src.data_ptr(), d_src.numel(), d_recs.data_ptr(), case.n,
                                     te.data_ptr() if te.numel() else res.data_ptr(), te.numel(), case.uuid, 3, 3,
                                     out.data_ptr() if cap else None, cap, 0, nr.data_ptr(), so.data_ptr(),
                                     sl.data_ptr(), res.data_ptr(), None, ctypes.byref(opts), 0,
                                     torch.cuda.current_stream(gpu).cuda_stream))
        r = res.cpu().numpy().view(np.uint64)
        assert [int(v) for v in r[:3]] == head, (name, r)
        tail = [len(base.want), base.n_commits, 0, 0, 0] if head[0] == lc.OVERFLOW else [0] * 5
        assert [int(v) for v in r[3:]] == tail, (name, r)
        assert bool((whole == CANARY).all()), name
        assert bool((nr == 0x5A5A).all() and (so == 0x5A5A).all() and (sl == 0x5A5A).all()), name


# ------------------------------------------------- through the existing stages
def test_lister_and_verifier_agree(gpu):
    names = ("alignment_grid_tx_of_7", "shared_bytes", "tx_two_deletes", "tx_mixed_empty", "count_4097", "key_65536",
             "finalise_after_tx", "three_empty_tx_finalise", "append_at_8_mod_16", "src_inside_out")
    cases = [c for c in lc.small_cases() if c.name in names]
    assert len(cases) == len(names)
    for case in cases:
        d, got = same(case, gpu)
        img = dm.dev_bytes(case.want, gpu)
        img.copy_(torch.from_numpy(got[:len(case.want)].copy()))
        recs, res = zsfile.device_records(img, zsfile.ACTIVE)
        lr = res.cpu().numpy().view(np.uint64)
        whole, rc = ri.host_records(case.want, zsfile.ACTIVE)
        assert int(lr[0]) == zsfile.END and int(lr[1]) == len(whole), case.name
        # the records of the call are the image's last n
        listed = recs[len(whole) - case.n:len(whole)].cpu().numpy().view(np.uint64)
        assert np.array_equal(listed, d["new_recs"]), case.name
        v, hv = zsfile.verify_device_image(img, zsfile.ACTIVE), zsfile.verify_image(case.want, zsfile.ACTIVE)
        assert v == hv, (case.name, v, hv)
        # every commit good but the stale finalise commits (hashed from a register that was not 0)
        off, ln, _, _ = zsfile.walk(case.want)
        assert v["n_commits"] == len(off) and v["walk_rc"] == zsfile.END
        stale = sum(1 for c in zf.walk(case.want)[0] if not c["ok"])
        assert v["n_bad"] == stale and stale <= (2 if case.at else 1) and (stale == 0 or case.finalise), case.name
        # the span descriptors feed the commit verifier without a walk
        if d["commits"]:
            so = torch.from_numpy(d["span_off"].view(np.int64).copy()).to(gpu)
            sl = torch.from_numpy(d["span_len"].view(np.int64).copy()).to(gpu)
            _, status = zsfile.verify_commits(img, so, sl)
            st = status.cpu().numpy()
            good = d["commits"] - (1 if case.finalise and d["last_crc"] != 0 else 0)
            assert int((st == 1).sum()) == good and bool((st[:good] == 1).all()), (case.name, st)


def test_log_append_list_merge_pack(gpu):
    """Batch A at 0, batch B appended (keys of A overwritten and deleted), then
    the lister, the merge and the packer: the packed file of the merged dict."""
    rng = np.random.default_rng(77)
    keys = [b"key-%05d" % i + b"x" * int(rng.integers(0, 20)) for i in range(600)]
    a = [(k, rng.integers(0, 256, int(rng.integers(0, 90)), dtype=np.uint8).tobytes()) for k in keys[:400]]
    b = []
    for i in rng.permutation(600)[:350]:
        b.append((keys[i], None if i % 3 == 0 else rng.integers(0, 256, int(rng.integers(0, 200)), dtype=np.uint8).tobytes()))
    merged = dict(a)
    merged.update(dict(b))
    ca, cb = pc.from_pairs("A", a, seed=1), pc.from_pairs("B", b, seed=2)
    cap = 1 << 20
    out = torch.full((cap,), CANARY, dtype=torch.uint8, device=gpu)
    da = zsfile.device_log(dm.dev_bytes(ca.src, gpu), dm.dev_recs(ca.recs, gpu), None, lc.UUID, 5, 5, out=out)
    ends = torch.tensor(list(range(7, len(b), 7)) + [len(b)], dtype=torch.int64, device=gpu)
    db = zsfile.device_log(dm.dev_bytes(cb.src, gpu, 3), dm.dev_recs(cb.recs, gpu), ends, out=out, at=da["end"], finalise=True)
    assert da["code"] == 0 and db["code"] == 0 and db["end"] > da["end"]
    img = db["image"]
    recs, res = zsfile.device_records(img, zsfile.ACTIVE)
    lr = res.cpu().numpy().view(np.uint64)
    assert int(lr[0]) == zsfile.END and int(lr[1]) == len(a) + len(b)
    won, mres = repack.device_merge(img, [(recs[:int(lr[1])], 0)])
    packed, pres = repack.device_pack(img, won, lc.UUID, 5, 5)
    assert int(pres[0]) == 0
    assert packed.cpu().numpy().tobytes() == zf.packed_file(sorted(merged.items()), lc.UUID, 5, 5)


# ------------------------------------------------------------------------ soak
def test_seeded_soak(gpu):
    """About 200 random small lists against the oracle: lengths, deletes,
    tables, at, FINALISE, prev_crc and tile at random; the user stream and the
    NULL stream, the library's scratch and the caller's take turns."""
    rng = np.random.default_rng(20260)
    side = torch.cuda.Stream(device=gpu)
    pres = [lc.earlier_image(False), lc.earlier_image(True)]
    for it in range(200):
        n = int(rng.integers(0, 60))
        lens = [(int(rng.integers(0, 70)), None if rng.integers(0, 4) == 0 else int(rng.integers(0, 300)))
                for _ in range(n)]
        mode = int(rng.integers(0, 3))
        if mode == 0 and n:
            ends = None
        else:
            ends, e = [], 0
            while e < n or (n == 0 and len(ends) < mode):
                e = min(n, e + int(rng.integers(0, 9)))
                ends.append(e)
        pre = pres[it % 2] if rng.integers(0, 2) else b""
        case = lc.from_lengths("soak_%d" % it, lens, seed=it, tx_end=ends, prefix=pre,
                               finalise=bool(rng.integers(0, 2)), prev_crc=int(rng.integers(0, 2 ** 32)))
        tile = int(rng.choice([0, 64, 128, 1024, 4096, 65536]))
        scratch = None
        if it % 2:
            need = zsfile.device_log_scratch_bytes(n, n if ends is None else len(ends), tile)
            whole, scratch = dm.fenced(need, gpu)
        torch.cuda.synchronize(gpu)
        if it % 4 < 2:
            with torch.cuda.stream(side):
                same(case, gpu, tile=tile, shift=it % 8, scratch=scratch)
        else:
            same(case, gpu, tile=tile, shift=it % 8, scratch=scratch)
        if scratch is not None:
            assert dm.intact(whole, need), it


# ---------------------------------------------------------------- beyond 4 GiB
def test_offsets_beyond_4gib(gpu):
    """A source and an output of 2^32 + 1 MiB bytes each, only their tails
    filled: key_off / val_off above 2^32, appended at at = 2^32 + 8.  The tail
    written equals the host twin's over the same bytes (the source tail with
    the offsets rebased, appended at 56: the same residue mod 16)."""
    B32, MIB = 1 << 32, 1 << 20
    free, _ = torch.cuda.mem_get_info(gpu)
    if free < 10 << 30:
        pytest.skip("a source and an output of 4 GiB + 1 MiB each need 10 GiB of free device memory, %.1f GiB are free"
                    % (free / 2 ** 30))
    rng = np.random.default_rng(99)
    tail = rng.integers(0, 256, MIB, dtype=np.uint8)
    n = 3000
    klen, vlen = rng.integers(0, 40, n), rng.integers(0, 250, n)
    koff, voff = rng.integers(0, MIB - 40, n), rng.integers(0, MIB - 250, n)
    recs = np.stack([koff, klen, voff, vlen], 1).astype(np.uint64)
    recs[::9, 2], recs[::9, 3] = lc.U64_MAX, 0
    ends = list(range(11, n, 11)) + [n]
    at_h = 56
    hout = np.full(MIB, CANARY, np.uint8)
    h = zsfile.log(tail, recs, ends, out=hout, at=at_h, finalise=True, prev_crc=7, new_recs=True, spans=True)
    assert h["code"] == 0 and h["end"] < MIB - 64

    d_src = torch.empty(B32 + MIB, dtype=torch.uint8, device=gpu)
    d_src[B32:].copy_(torch.from_numpy(tail))
    d_out = torch.empty(B32 + MIB, dtype=torch.uint8, device=gpu)
    d_out[B32 - 4096:].fill_(CANARY)
    at = B32 + 8
    big = recs.copy()
    big[:, 0] += np.uint64(B32)
    big[big[:, 2] != lc.U64_MAX, 2] += np.uint64(B32)
    assert int(big[:, 0].min()) >= B32
    d = zsfile.device_log(d_src, dm.dev_recs(big, gpu), torch.tensor(ends, dtype=torch.int64, device=gpu), out=d_out,
                          at=at, finalise=True, prev_crc=7, new_recs=True, spans=True)
    shift = at - at_h
    assert d["code"] == 0 and d["end"] == h["end"] + shift and d["written"] == h["written"]
    assert [d[k] for k in WORDS[4:]] == [h[k] for k in WORDS[4:]]
    got = d_out[B32 - 4096:].cpu().numpy()
    assert bool((got[:4096 + 8] == CANARY).all())                               # nothing before at
    w = h["written"]
    assert got[4096 + 8:4096 + 8 + w].tobytes() == hout[at_h:at_h + w].tobytes()
    assert bool((got[4096 + 8 + w:] == CANARY).all())                           # nothing at or after the end
    nr, hr = d["new_recs"].cpu().numpy().view(np.uint64), np.asarray(h["new_recs"]).copy()
    live = hr[:, 2] != lc.U64_MAX
    hr[:, 0] += np.uint64(shift)
    hr[live, 2] += np.uint64(shift)
    assert np.array_equal(nr, hr)
    assert np.array_equal(d["span_off"].cpu().numpy().view(np.uint64), np.asarray(h["span_off"]) + np.uint64(shift))
    assert np.array_equal(d["span_len"].cpu().numpy().view(np.uint64), np.asarray(h["span_len"]))
