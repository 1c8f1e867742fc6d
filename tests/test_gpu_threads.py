"""libzscrc called from several host threads at once, and on the stream
handles that are not ordinary streams.

The library's per-device state is shared by every caller: the class lists and
part registers of variable batches, the span scratch, qteam_dyn's part
registers, the verdict counter pairs, nbv's part registers, the walk's
scratch, the host-batch staging and the scalar offload's cached stream
(zscrc_api.cpp DevCtx, zscrc_scratch.cpp Scratch).  Calls that use it are
enqueued under a lock and ordered across streams by an event; the code that
decides whether two calls are on one stream compares stream handles -- and
hipStreamPerThread is ONE handle for a different stream in every thread.

test_threads: four Python threads call the C ABI through ctypes (which drops
the GIL, so the calls overlap), a start barrier the only synchronisation
between them, six rounds of every operation of the table in DESIGN.md §7
each.  Every input, output buffer and expected value (the CPU oracle's, the
format oracle's; the walk against zscrc_zs_walk) exists before the threads
start; a single-threaded pass of every operation first brings all library
scratch to its final size.  All threads' inputs have the same shapes (sizes,
counts, caps, image sizes, walk geometry) and differ in their bytes only, so
a missed ordering shows as a wrong value inside the thread's own buffers.
Asynchronous results are read after the join and a device synchronise,
synchronous ones compared in the calling thread.  Stream modes: a side
stream per thread, one side stream for all, NULL, and hipStreamPerThread.
Afterwards every operation runs once more on the default stream: counters
and events are at rest.  (Equal shapes do not make every missed ordering
harmless: with handles compared for equality, the per-thread mode ran the
threads' classify launches at once on the shared class lists and the device
reported an illegal memory access -- the lists' scatter cursors are shared
too.  same_stream() in zscrc_internal.h is the fix.)

test_verdicts_on_seventy_streams: more streams than the 64 that get verdict
counter pairs (verdict_slot's fallback).  test_cpass_create_beside_a_side_
stream: zscrc_cpass_create while the lengths are still being written on a
non-blocking stream -- the caller's max_len must hold.
test_cpass_passes_on_special_handles: consecutive passes of one handle on
hipStreamPerThread, a side stream, hipStreamLegacy and NULL."""
import ctypes
import threading

import numpy as np
import pytest
import torch

from oracle import oracle
from oracle import zs_format as zf
from tests import walk_images as wi
from tests.images import UUID
from tests.images import oracle_bad as _oracle_bad
from zeroskip_amd import zsfile
from zeroskip_amd._lib import LEN_UNBOUNDED, check, lib, stats

pytestmark = pytest.mark.gpu

HIP_STREAM_PER_THREAD = 2   # hip_runtime_api.h: #define hipStreamPerThread ((hipStream_t)2)
HIP_STREAM_LEGACY = 1       # hip_runtime_api.h: #define hipStreamLegacy ((hipStream_t)1)
NT, ROUNDS = 4, 6
SLOTS = ROUNDS + 1          # output slot ROUNDS: the warm-up pass, then the pass after the join
QDEAL, QFOLD = 1 << 25, 32  # zs::BatchDesc::opt (tests/test_gpu_parity.py): qteam_dyn_kernel, its fold a launch
FIXED_N, FIXED_LEN = 16387, 2048
SPAN_LEN, SPAN_OFF = (3 << 20) + 7, 3
SPANS = [(100, 20000), (50000, 70001), (1 << 20, 300000)]   # (offset, length), each >= 16 KiB
SCALAR_LEN = 5 << 20
STREAM_LEN, STREAM_CHUNK = 9 << 20, 4 << 20
HOST_N = 500
WALK_BLOCK, WALK_TILE = 8192, 1024
CAP = 64                    # verdict list entries


# ------------------------------------------------------------------ inputs
def _schedules():
    """The shapes every thread shares: value sizes of every transaction."""
    rng = np.random.default_rng(1)
    short = [list(rng.integers(0, 150, int(rng.integers(1, 3)))) for _ in range(3000)]
    mixed = []
    for _ in range(300):
        p = rng.random()
        mixed.append([int(rng.integers(0, 500))] if p < 0.7 else [int(rng.integers(2000, 20000))] if p < 0.9
                     else [int(rng.integers(50000, 150000))])
    mixed[17] = [1 << 20, 200_000]       # a class-3 commit
    mixed[250] = [1 << 20, 150_000]
    long = [[1 << 20, int(rng.integers(100_000, 500_000))] for _ in range(8)]
    walk = [list(rng.integers(0, 40, int(rng.integers(1, 4)))) for _ in range(700)]
    return dict(short=short, mixed=mixed, long=long, walk=walk)


def _log(schedule, seed):
    """An active file of the schedule's transactions: the same offsets and
    lengths for every seed, other value bytes."""
    rng = np.random.default_rng(seed)
    w = zf.FileWriter(UUID, idx=0)
    for t, txn in enumerate(schedule):
        for k, v in enumerate(txn):
            w.add(b"%07d-%04d" % (t, k), rng.integers(0, 256, int(v), dtype=np.uint8).tobytes())
        w.commit()
    return np.frombuffer(w.image(), np.uint8).copy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class VerdictCase:
    """A corrupted image, its commits plus entries outside the image, and
    the indices the format oracle rejects."""

    def __init__(self, clean, seed, hits, outside):
        cs = zf.walk(clean.tobytes())[0]
        self.clean, self.commits = clean, cs
        offs = [c["span_off"] for c in cs]
        lens = [c["span_len"] for c in cs]
        rng = np.random.default_rng(seed)
        img = clean.copy()
        for i in rng.choice(len(cs), hits, replace=False):
            if lens[i] and rng.random() < 0.7:
                img[offs[i] + int(rng.integers(0, lens[i]))] ^= 0x5A
            else:
                img[cs[i]["commit_off"] + 4 + int(rng.integers(0, 4))] ^= 0x01
        size = img.nbytes
        for back, ln in outside:          # the same entries in every thread
            offs.append(size - back)
            lens.append(ln)
        self.host = img
        self.offs, self.lens = np.array(offs, np.int64), np.array(lens, np.int64)
        self.want = _oracle_bad(img, self.offs, self.lens, None)
        assert len(self.want) >= hits // 2 + len(outside) and len(self.want) <= CAP
        self.n = len(offs)
        self.d, self.o, self.ln = _dev(img), _dev(self.offs), _dev(self.lens)
        self.nbad = [torch.full((1,), -1, dtype=torch.int64, device="cuda") for _ in range(SLOTS)]
        self.bad = [torch.full((CAP,), -1, dtype=torch.int64, device="cuda") for _ in range(SLOTS)]

    def mismatch(self, slot):
        k = int(self.nbad[slot].item())
        got = set(self.bad[slot][:max(0, min(k, CAP))].cpu().tolist())
        return None if (k, got) == (len(self.want), self.want) else (k, sorted(got)[:8], len(self.want))


class Inputs:
    """Everything thread t reads or writes."""

    def __init__(self, t, sched):
        s = 1000 * (t + 1)
        rng = np.random.default_rng(s)
        # the batch of test_two_streams_share_scratch; lengths from the shared shape
        lens = np.random.default_rng(21).integers(0, 3000, 3000).astype(np.uint64)
        lens[:3] = [5 << 20, 3 << 20, 70000]
        offs = np.zeros(3000, np.uint64)
        offs[1:] = np.cumsum(lens[:-1])
        self.host = rng.integers(0, 256, int(offs[-1] + lens[-1]), dtype=np.uint8)
        assert self.host.nbytes >= max(STREAM_LEN, SCALAR_LEN + 1, SPAN_OFF + SPAN_LEN)
        self.b_offs, self.b_lens = offs, lens
        self.b_want = oracle.batch(self.host, offs, lens, impl="hw", threads=8)
        self.data, self.d_off, self.d_len = _dev(self.host), _dev(offs.astype(np.int64)), _dev(lens.astype(np.int64))
        self.b_out = [torch.zeros(3000, dtype=torch.int32, device="cuda") for _ in range(SLOTS)]
        # one span, library scratch; three spans in one launch pair
        self.span_want = oracle.crc32c_hw(0, self.host[SPAN_OFF:SPAN_OFF + SPAN_LEN])
        self.span_out = [torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(SLOTS)]
        self.spans_ptr = (ctypes.c_void_p * 3)(*[self.data.data_ptr() + o for o, _ in SPANS])
        self.spans_len = (ctypes.c_uint64 * 3)(*[n for _, n in SPANS])
        self.spans_want = [oracle.crc32c_hw(0, self.host[o:o + n]) for o, n in SPANS]
        self.spans_out = [torch.zeros(3, dtype=torch.int32, device="cuda") for _ in range(SLOTS)]
        # fixed-stride records on qteam_dyn_kernel
        fh = rng.integers(0, 256, FIXED_N * FIXED_LEN, dtype=np.uint8)
        self.fixed = _dev(fh)
        self.fixed_want = oracle.batch(fh, n=FIXED_N, stride=FIXED_LEN, fixed_len=FIXED_LEN, impl="hw", threads=8)
        self.fixed_out = [torch.zeros(FIXED_N, dtype=torch.int32, device="cuda") for _ in range(SLOTS)]
        # verdicts: bounded (the counter pairs), unbounded over mixed lengths (classify), long only (nbv)
        short = _log(sched["short"], s + 1)
        self.short = VerdictCase(short, s + 2, 16, [(100, 300), (-64, 50)])
        assert self.short.lens.max() <= 640
        self.mixed = VerdictCase(_log(sched["mixed"], s + 3), s + 4, 12, [(1000, 5000), (-64, 50)])
        assert self.mixed.lens.max() > (1 << 20) and self.mixed.lens.min() <= 640
        long = _log(sched["long"], s + 5)
        first = zf.walk(long.tobytes())[0][0]["span_len"]
        self.long = VerdictCase(long, s + 6, 2, [(1000, first)])
        self.lo, self.hi = int(self.long.lens.min()), int(self.long.lens.max())
        assert self.lo > (1 << 20)
        # the writer: the clean short image with every CRC field zeroed
        cs = self.short.commits
        blank = short.copy()
        at = np.array([c["commit_off"] + 4 for c in cs])
        blank[(at[:, None] + np.arange(4)).reshape(-1)] = 0
        assert not np.array_equal(blank, short)
        self.w_want, self.w_n = short, len(cs)
        self.w_blank = _dev(blank)
        self.w_img = [_dev(blank) for _ in range(SLOTS)]
        # the device walk on a multi-block image (and the same image verified whole)
        wimg = _log(sched["walk"], s + 7)
        bad_at = zf.walk(wimg.tobytes())[0][40 + t]
        wimg[bad_at["span_off"] + 1] ^= 0x04
        assert wimg.nbytes > 4 * WALK_BLOCK
        self.walk_host, self.walk = wimg, _dev(wimg)
        self.walk_want = wi.host_walk(wimg)
        self.walk_cap = len(self.walk_want[0]) + 8
        self.walk_out = [(torch.full((self.walk_cap,), -1, dtype=torch.int64, device="cuda"),
                          torch.full((self.walk_cap,), -1, dtype=torch.int64, device="cuda"),
                          torch.full((zsfile.WALK_RES_WORDS,), -1, dtype=torch.int64, device="cuda"))
                         for _ in range(SLOTS)]
        self.walk_opts = zsfile.WalkOpts(WALK_BLOCK, WALK_TILE)
        commits, end, why = zf.walk(wimg.tobytes())
        bad = [i for i, c in enumerate(commits) if not c["ok"]]
        assert why == "end" and bad == [40 + t] and zf.header_check(wimg.tobytes())[0]
        self.image_want = dict(header_rc=0, walk_rc=zsfile.END, end_off=end, n_commits=len(commits), n_bad=1,
                               first_bad=bad[0])
        # host batch, scalar offload, host byte stream
        self.h_off = np.ascontiguousarray(offs[3:3 + HOST_N])
        self.h_len = np.ascontiguousarray(lens[3:3 + HOST_N])
        self.h_want = self.b_want[3:3 + HOST_N]
        self.h_out = np.zeros(HOST_N, np.uint32)
        self.scalar_want = oracle.crc32c_hw(0, self.host[1:1 + SCALAR_LEN])
        self.stream_seed = 0x51 + t
        self.stream_want = oracle.crc32c_hw(self.stream_seed, self.host[:STREAM_LEN])


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def one_pass(x: Inputs, slot: int, stream, errors: list, tag):
    """Every operation once for the inputs x: asynchronous ones into output
    slot `slot` on `stream`, synchronous ones compared here."""
    L = lib()
    check(L.zscrc_device_batch(x.data.data_ptr(), x.d_off.data_ptr(), x.d_len.data_ptr(), None,
                               x.b_out[slot].data_ptr(), 3000, 0, stream), "device_batch")
    check(L.zscrc_device_span(x.data.data_ptr() + SPAN_OFF, SPAN_LEN, 0, x.span_out[slot].data_ptr(), None, 0,
                              stream), "device_span")
    check(L.zscrc_device_spans(ctypes.addressof(x.spans_ptr), ctypes.addressof(x.spans_len), None,
                               x.spans_out[slot].data_ptr(), 3, 0, stream), "device_spans")
    check(L.zscrc_device_fixed(x.fixed.data_ptr(), FIXED_LEN, FIXED_LEN, 0, x.fixed_out[slot].data_ptr(), FIXED_N, 0,
                               stream), "device_fixed")
    v = x.short
    check(L.zscrc_device_verify_commits_verdict(v.d.data_ptr(), v.host.nbytes, v.o.data_ptr(), v.ln.data_ptr(), None,
                                                v.n, 640, v.nbad[slot].data_ptr(), v.bad[slot].data_ptr(), CAP,
                                                stream), "verdict (bounded)")
    v = x.mixed
    check(L.zscrc_device_verify_commits_verdict(v.d.data_ptr(), v.host.nbytes, v.o.data_ptr(), v.ln.data_ptr(), None,
                                                v.n, LEN_UNBOUNDED, v.nbad[slot].data_ptr(), v.bad[slot].data_ptr(),
                                                CAP, stream), "verdict (unbounded)")
    v = x.long
    check(L.zscrc_device_verify_commits_verdict_range(v.d.data_ptr(), v.host.nbytes, v.o.data_ptr(), v.ln.data_ptr(),
                                                      None, v.n, x.lo, x.hi, v.nbad[slot].data_ptr(),
                                                      v.bad[slot].data_ptr(), CAP, stream), "verdict_range")
    check(L.zscrc_device_write_commits(x.w_img[slot].data_ptr(), x.w_want.nbytes, x.short.o.data_ptr(),
                                       x.short.ln.data_ptr(), x.w_n, None, None, stream), "write_commits")
    off, ln, res = x.walk_out[slot]
    check(L.zscrc_device_walk(x.walk.data_ptr(), x.walk_host.nbytes, off.data_ptr(), ln.data_ptr(), x.walk_cap,
                              res.data_ptr(), None, ctypes.byref(x.walk_opts), 0, stream), "device_walk")
    # synchronous calls
    x.h_out[:] = 0
    check(L.zscrc_host_batch(x.host.ctypes.data, x.h_off.ctypes.data, x.h_len.ctypes.data, None, x.h_out.ctypes.data,
                             HOST_N), "host_batch")
    if not np.array_equal(x.h_out, x.h_want):
        errors.append((tag, "host_batch", int((x.h_out != x.h_want).sum())))
    got = L.crc32c_hw(0, x.host.ctypes.data + 1, SCALAR_LEN)
    if got != x.scalar_want:
        errors.append((tag, "crc32c_hw", hex(got), hex(x.scalar_want)))
    h = ctypes.c_void_p()
    check(L.zscrc_stream_open(ctypes.byref(h), x.stream_seed, STREAM_CHUNK, 0), "stream_open")
    rc = 0
    for k in range(3):
        rc = rc or L.zscrc_stream_update(h, x.host.ctypes.data + k * (STREAM_LEN // 3), STREAM_LEN // 3)
    crc = ctypes.c_uint32()
    rc2 = L.zscrc_stream_final(h, ctypes.byref(crc))    # always frees the stream
    check(rc or rc2, "stream_update / final")
    if crc.value != x.stream_want:
        errors.append((tag, "zscrc_stream", hex(crc.value), hex(x.stream_want)))
    rep = zsfile.Report()
    check(L.zscrc_device_verify_image(x.walk.data_ptr(), x.walk_host.nbytes, zsfile.ACTIVE, ctypes.byref(rep), stream),
          "device_verify_image")
    got = {k: getattr(rep, k) for k in x.image_want}
    if got != x.image_want or rep.header_stored != rep.header_computed:
        errors.append((tag, "device_verify_image", got, x.image_want))


def compare(x: Inputs, slot: int, errors: list, tag):
    """The asynchronous results of output slot `slot` (the device is idle)."""
    def bad(name, ok, *what):
        if not ok:
            errors.append((tag, name, *what))
    bad("device_batch", np.array_equal(_u32(x.b_out[slot]), x.b_want))
    bad("device_span", int(_u32(x.span_out[slot])[0]) == x.span_want)
    bad("device_spans", _u32(x.spans_out[slot]).tolist() == x.spans_want)
    bad("device_fixed", np.array_equal(_u32(x.fixed_out[slot]), x.fixed_want))
    for name, v in (("verdict (bounded)", x.short), ("verdict (unbounded)", x.mixed), ("verdict_range", x.long)):
        m = v.mismatch(slot)
        bad(name, m is None, m)
    bad("write_commits", np.array_equal(x.w_img[slot].cpu().numpy(), x.w_want))
    off, ln, res = (a.cpu().numpy() for a in x.walk_out[slot])
    w_off, w_len, w_rc, w_end = x.walk_want
    n = len(w_off)
    bad("device_walk", (int(res[0]), int(res[1]), int(res[2])) == (w_rc, n, w_end) and
        np.array_equal(off[:n].astype(np.uint64), w_off) and np.array_equal(ln[:n].astype(np.uint64), w_len) and
        (off[n:] == -1).all(), res.tolist())


@pytest.fixture(scope="module")
def inputs(gpu):
    sched = _schedules()
    xs = [Inputs(t, sched) for t in range(NT)]
    for a, b in zip(xs, xs[1:]):       # equal shapes, other bytes
        for name in ("short", "mixed", "long"):
            va, vb = getattr(a, name), getattr(b, name)
            assert np.array_equal(va.offs, vb.offs) and np.array_equal(va.lens, vb.lens)
            assert va.host.nbytes == vb.host.nbytes and not np.array_equal(va.host, vb.host)
        assert a.walk_host.nbytes == b.walk_host.nbytes and a.walk_cap == b.walk_cap
        assert a.host.nbytes == b.host.nbytes
    torch.cuda.synchronize()
    return xs


@pytest.fixture
def tuned(gpu):
    """What the threads only read: the QDEAL form of zscrc_device_fixed and a
    scalar offload threshold of one byte, set before they start."""
    L = lib()
    warm, cold = L.zscrc_gpu_min(0), L.zscrc_gpu_min(1)
    L.zscrc_set_opt(QDEAL | QFOLD)
    L.zscrc_set_gpu_min(1)
    try:
        yield
    finally:
        L.zscrc_set_opt(0)
        L.zscrc_set_gpu_min_pair(warm, cold)


@pytest.mark.parametrize("mode", ["own", "shared", "null", "per_thread"])
def test_threads(inputs, tuned, mode):
    xs = inputs
    name = lib().zscrc_fixed_kernel(xs[0].fixed.data_ptr(), FIXED_LEN, FIXED_LEN, FIXED_N).decode()
    assert name == "qteam_dyn_kernel+qfold_kernel", name
    side = [torch.cuda.Stream() for _ in range(NT)]      # alive until the end of the test
    handle = {"own": [s.cuda_stream for s in side], "shared": [side[0].cuda_stream] * NT, "null": [None] * NT,
              "per_thread": [HIP_STREAM_PER_THREAD] * NT}[mode]
    errors = []

    def reset(slots):
        for x in xs:
            for slot in slots:
                for t in (x.b_out, x.span_out, x.spans_out, x.fixed_out):
                    t[slot].zero_()
                for v in (x.short, x.mixed, x.long):
                    v.nbad[slot].fill_(-1)
                    v.bad[slot].fill_(-1)
                for a in x.walk_out[slot]:
                    a.fill_(-1)
                x.w_img[slot].copy_(x.w_blank)
        torch.cuda.synchronize()

    # single-threaded warm-up of every operation: all library scratch at its final size
    reset(range(SLOTS))
    before = stats()
    for t, x in enumerate(xs):
        one_pass(x, ROUNDS, None, errors, ("warm-up", t))
    torch.cuda.synchronize()
    per_pass = (stats()[0] + stats()[1] - before[0] - before[1]) // NT
    for t, x in enumerate(xs):
        compare(x, ROUNDS, errors, ("warm-up", t))
    assert not errors, errors[:6]
    reset([ROUNDS])

    start = threading.Barrier(NT)
    failed = []

    def body(t):
        try:
            start.wait()
            for r in range(ROUNDS):
                one_pass(xs[t], r, handle[t], errors, (mode, t, r))
        except Exception as e:  # noqa: BLE001 -- reported by the main thread
            failed.append((t, repr(e)))

    before = stats()
    threads = [threading.Thread(target=body, args=(t,)) for t in range(NT)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    torch.cuda.synchronize()
    after = stats()
    assert not failed, failed
    for t, x in enumerate(xs):
        for r in range(ROUNDS):
            compare(x, r, errors, (mode, t, r))
    assert not errors, (len(errors), errors[:8])
    # every scalar call counted once, on the CPU ([0]: the offload was busy) or
    # on the GPU ([1]): per pass one crc32c_hw here plus the library's own of
    # device_verify_image's header check, the same number in every pass
    assert per_pass >= 1
    assert after[0] + after[1] - before[0] - before[1] == NT * ROUNDS * per_pass

    # at rest: every operation once more on the default stream
    before = stats()
    for t, x in enumerate(xs):
        one_pass(x, ROUNDS, torch.cuda.current_stream().cuda_stream, errors, ("after", t))
    torch.cuda.synchronize()
    assert stats()[0] + stats()[1] - before[0] - before[1] == NT * per_pass
    for t, x in enumerate(xs):
        compare(x, ROUNDS, errors, ("after", t))
    assert not errors, errors[:6]


# ------------------------------------------------------- deterministic tests
def test_verdicts_on_seventy_streams(inputs):
    """64 stream handles get verdict counter pairs; the 65th and later take
    the fallback (the caller's counter zeroed by a memset on the stream).
    One bounded verdict on each of 70 live streams, none waited for until all
    are queued, then one more on the first: every count and list is the
    oracle's."""
    v = inputs[0].short
    streams = [torch.cuda.Stream() for _ in range(70)]
    outs = [(torch.full((1,), -1, dtype=torch.int64, device="cuda"),
             torch.full((CAP,), -1, dtype=torch.int64, device="cuda")) for _ in range(71)]
    torch.cuda.synchronize()
    for (nbad, bad), s in zip(outs, streams + streams[:1]):
        check(lib().zscrc_device_verify_commits_verdict(v.d.data_ptr(), v.host.nbytes, v.o.data_ptr(), v.ln.data_ptr(),
                                                        None, v.n, 640, nbad.data_ptr(), bad.data_ptr(), CAP,
                                                        s.cuda_stream), "verdict (bounded)")
    torch.cuda.synchronize()
    for j, (nbad, bad) in enumerate(outs):
        k = int(nbad.item())
        assert k == len(v.want) and set(bad[:k].cpu().tolist()) == v.want, (j, k, len(v.want))


def test_cpass_create_beside_a_side_stream(gpu):
    """zscrc_cpass_create reads d_len back with a blocking copy on the NULL
    stream, which a non-blocking stream (every torch side stream) is not
    ordered before: with the true lengths still being written there it reads
    stale short ones.  The caller's max_len -- the host walk's, the true
    maximum -- must then be the bound the verdict runs with: the corrupted
    longest commit is listed."""
    from tests.consistent_cases import small_db
    from zeroskip_amd import consistent as cs
    from zeroskip_amd import device as zd
    job = cs.Consistent(cs.open_db(small_db(long_region=True)), 0, 1).prepare()
    i = int(torch.argmax(job.d_len))
    L = int(job.d_len[i])
    assert L > 640
    job.buf[int(job.d_off[i]) + L // 2] ^= 0x21
    true = job.d_len.cpu().pin_memory()
    job.d_len.copy_(torch.clamp(job.d_len, max=64))        # stale lengths, all <= 64
    busy = torch.empty(1 << 30, dtype=torch.uint8, device=gpu)
    busy.random_(0, 256)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    h = ctypes.c_void_p()
    res = cs.CPassResult()
    with torch.cuda.device(job.buf.device):
        with torch.cuda.stream(side):
            for _ in range(150):                            # ~0.2 ms each: tens of milliseconds queued
                zd.crc_span(busy)
            job.d_len.copy_(true, non_blocking=True)
        spec = cs.CPassSpec(job.buf.data_ptr(), job.buf.numel(), len(job.c_off), job.d_off.data_ptr(),
                            job.d_len.data_ptr(), job.d_file.data_ptr(), L, 0, None, None, None)
        check(lib().zscrc_cpass_create(ctypes.byref(h), ctypes.byref(spec)), "zscrc_cpass_create")
        try:
            torch.cuda.synchronize()
            assert int(job.d_len[i]) == L
            check(lib().zscrc_cpass_run(h, None, ctypes.byref(res)), "zscrc_cpass_run")
        finally:
            lib().zscrc_cpass_destroy(h)
    bad = list(res.bad[:res.n_listed_bad])
    assert res.complete and i in bad, (i, bad, res.n_bad)


def test_cpass_passes_on_special_handles(gpu):
    """Each pass of a zscrc_cpass zeroes the counters the next one increments,
    so passes follow one another in stream order: a pass on another stream
    than the previous one waits for it.  Two passes in flight at a time
    (submit / collect) over hipStreamPerThread, a side stream,
    hipStreamLegacy, NULL and the per-thread handle twice in a row: every
    result is the first, synchronous one's, which lists the corrupted commit
    -- counted once per pass."""
    from tests.consistent_cases import small_db
    from zeroskip_amd import consistent as cs
    job = cs.Consistent(cs.open_db(small_db(long_region=True)), 0, 1).prepare()
    i = int(torch.argmax(job.d_len))
    L = int(job.d_len[i])
    job.buf[int(job.d_off[i]) + L // 2] ^= 0x21
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    h = ctypes.c_void_p()
    spec = cs.CPassSpec(job.buf.data_ptr(), job.buf.numel(), len(job.c_off), job.d_off.data_ptr(),
                        job.d_len.data_ptr(), job.d_file.data_ptr(), L, 0, None, None, None)

    def summary(res):
        return (res.complete, res.n_bad, res.n_stale, res.n_undecided, list(res.bad[:res.n_listed_bad]),
                list(res.stale[:res.n_listed_stale]))

    with torch.cuda.device(job.buf.device):
        check(lib().zscrc_cpass_create(ctypes.byref(h), ctypes.byref(spec)), "zscrc_cpass_create")
        try:
            first = cs.CPassResult()
            check(lib().zscrc_cpass_run(h, None, ctypes.byref(first)), "zscrc_cpass_run")
            want = summary(first)
            assert want[0] and want[1] >= 1 and i in want[4], want
            handles = [HIP_STREAM_PER_THREAD, side.cuda_stream, HIP_STREAM_LEGACY, None, HIP_STREAM_PER_THREAD,
                       HIP_STREAM_PER_THREAD, side.cuda_stream, HIP_STREAM_PER_THREAD]
            got = []
            for k, s in enumerate(handles):
                slot = k % 2
                if k >= 2:
                    res = cs.CPassResult()
                    check(lib().zscrc_cpass_collect(h, slot, ctypes.byref(res)), "zscrc_cpass_collect")
                    got.append(summary(res))
                check(lib().zscrc_cpass_submit(h, s, None, None, slot), "zscrc_cpass_submit")
            for slot in (len(handles) % 2, (len(handles) + 1) % 2):
                res = cs.CPassResult()
                check(lib().zscrc_cpass_collect(h, slot, ctypes.byref(res)), "zscrc_cpass_collect")
                got.append(summary(res))
        finally:
            lib().zscrc_cpass_destroy(h)
    assert len(got) == len(handles) and all(g == want for g in got), (want, got)
