"""Rate of the device lookup (zscrc_device_find) in the 3,355,443 records of a
1 GiB device-resident log image of config 4's record shape (tools/zsdb_gen.py:
the image tools/probes/pack_rate.py builds), listed on the device -- its keys
ascend strictly, so the list is its own merged list (CHECK_ORDER says so).
Three query batches:
  random  1 M 16-byte keys in random order, half of them keys of the list, half
          such keys with their last byte flipped (a few of those may exist too:
          the result words count what was found)
  sorted  the same keys in the list's order
  own     the list's own records as queries, in order
each at splitters 1 (no table), 64, 2048 and the default (--sweep: 16, 256,
512 and 1024 too), interleaved in one run, against
  (b) what the call replaces: the list, the source and the keys copied to
      pinned host memory, then zscrc_zs_find on one core of the same machine;
  (c) context only: torch.searchsorted of as many int64 in a sorted int64
      array of as many entries, a search that never looks at key bytes.
Every table size's hits are compared with the no-table form's, and batch
`own` with the records' own indices.

The timing step runs twice, each a process of its own under its own time
limit; a row holds both runs' medians and their spread.  One JSON line per
batch and table size goes to --out (default profiles/find/find_rate.jsonl).
usage (GPU box): python tools/probes/find_rate.py [--out FILE] [--mib 1024]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tools.probes.pack_rate import build_image, listed, median  # noqa: E402

SPLITS = [1, 64, 2048, 0]
WARM, RUNS = 3, 17
NQ = 1 << 20


def batches(img, recs, n):
    """{name: (qsrc, queries)} on the device."""
    import torch
    dev = img.device
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    idx = torch.randint(0, n, (NQ,), generator=gen, device=dev)
    assert bool((recs[:, 1] == 16).all())
    keys = img[(recs[idx, 0][:, None] + torch.arange(16, device=dev)[None, :])]
    keys[NQ // 2:, 15] ^= 0xFF
    q = torch.zeros((NQ, 4), dtype=torch.int64, device=dev)
    q[:, 0] = 16 * torch.arange(NQ, device=dev)
    q[:, 1] = 16
    order = torch.argsort(idx, stable=True)
    return {"random": (keys.reshape(-1).contiguous(), q),
            "sorted": (keys[order].reshape(-1).contiguous(), q),
            "own": (img, recs)}


def step_time(args):
    import numpy as np
    import torch
    from zeroskip_amd import zsfile
    img, pairs = build_image(args.mib)
    dev = img.device
    size = img.numel()
    recs, n, _ = listed(img, pairs)
    recs = recs.contiguous()
    level = [(recs, 0)]
    rows = []
    host_src = None
    for name, (qsrc, q) in batches(img, recs, n).items():
        nq = int(q.shape[0])
        out = {s: (torch.empty((nq, 4), dtype=torch.int64, device=dev), torch.empty(8, dtype=torch.int64, device=dev))
               for s in SPLITS}
        ms = {s: [] for s in SPLITS}
        for it in range(WARM + RUNS):
            for s in SPLITS:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                zsfile.device_find(img, level, qsrc, q, splitters=s, out=out[s])
                e1.record()
                torch.cuda.synchronize()
                if it >= WARM:
                    ms[s].append(e0.elapsed_time(e1))
        # once with the order check: the list ascends strictly
        _, cres = zsfile.device_find(img, level, qsrc, q, check_order=True)
        res = out[1][1].cpu().tolist()
        assert res[0] == 0 and res[1] == nq and cres.cpu().tolist() == res, (name, res)
        equal = {s: bool(torch.equal(out[s][0], out[1][0]) and torch.equal(out[s][1], out[1][1])) for s in SPLITS}
        assert all(equal.values()), (name, equal)
        if name == "own":
            assert res[2] + res[3] == n and bool(torch.equal(out[1][0][:, 1], torch.arange(n, device=dev)))
        # (c) context: a search of as many int64 that never looks at key bytes
        hay = torch.arange(n, device=dev, dtype=torch.int64) * 2
        vals = torch.randint(0, 2 * n, (nq,), device=dev, dtype=torch.int64)
        if name != "random":
            vals = torch.sort(vals).values
        ss = []
        for it in range(WARM + RUNS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.searchsorted(hay, vals)
            e1.record()
            torch.cuda.synchronize()
            if it >= WARM:
                ss.append(e0.elapsed_time(e1))
        # (b) what the call replaces: list, source and keys to the host, one core's search
        d2h = []
        moved = [recs, img] if qsrc is img else [recs, img, qsrc, q]
        pins = [torch.empty(t.shape, dtype=t.dtype).pin_memory() for t in moved]
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for p, t in zip(pins, moved):
                p.copy_(t, non_blocking=True)
            torch.cuda.synchronize()
            d2h.append((time.perf_counter() - t0) * 1e3)
        del pins
        if host_src is None:
            host_src = (img.cpu().numpy(), recs.cpu().numpy())
        h_qsrc, h_q = (host_src if qsrc is img else (qsrc.cpu().numpy(), q.cpu().numpy()))
        t0 = time.perf_counter()
        hh, hres = zsfile.find(host_src[0], [(host_src[1], 0)], h_qsrc, h_q)
        host_ms = (time.perf_counter() - t0) * 1e3
        same_host = bool(np.array_equal(hh, out[1][0].cpu().numpy())) and hres.tolist() == res
        assert same_host, name
        for s in SPLITS:
            med = median(ms[s])
            rows.append({"probe": "find_rate", "image_bytes": size, "records": n, "batch": name, "queries": nq,
                         "splitters": s, "runs": len(ms[s]), "find_ms_median": round(med, 4),
                         "find_ms_min": round(min(ms[s]), 4), "find_ms_max": round(max(ms[s]), 4),
                         "mquery_s": round(nq / med / 1e3, 1), "res": res,
                         "scratch_bytes": zsfile.device_find_scratch_bytes(1, s),
                         "today": {"d2h_ms": round(median(d2h), 3), "host_find_ms_one_core": round(host_ms, 3),
                                   "total_ms": round(median(d2h) + host_ms, 3)},
                         "today_over_find": round((median(d2h) + host_ms) / med, 1),
                         "context": {"torch_searchsorted_int64_ms": round(median(ss), 4)},
                         "find_over_searchsorted": round(med / median(ss), 2),
                         "equal_to_no_table": equal[s], "equal_to_host": same_host})
    with open(args.tmp, "w") as f:
        json.dump(rows, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "find", "find_rate.jsonl"))
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--step", choices=["time"])
    ap.add_argument("--tmp")
    ap.add_argument("--sweep", action="store_true", help="also 16, 256, 512 and 1024 splitters")
    args = ap.parse_args()
    if args.sweep:
        SPLITS[:] = [1, 16, 64, 256, 512, 1024, 2048, 0]
    if args.step:
        return step_time(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__), "--mib", str(args.mib)] + (["--sweep"] if args.sweep else [])
    runs = []
    with tempfile.TemporaryDirectory(prefix="find_rate_") as work:
        for r in range(2):
            tmp = os.path.join(work, "time%d.json" % r)
            subprocess.run(["timeout", "-k", "10", "400"] + me + ["--step", "time", "--tmp", tmp], check=True)
            runs.append(json.load(open(tmp)))
    with open(args.out, "w") as f:
        for a, b in zip(*runs):
            assert (a["batch"], a["splitters"]) == (b["batch"], b["splitters"])
            lo, hi = sorted((a["find_ms_median"], b["find_ms_median"]))
            a["find_ms_median_runs"] = [a["find_ms_median"], b["find_ms_median"]]
            a["run_to_run_spread"] = round(hi / lo - 1, 4)
            f.write(json.dumps(a) + "\n")
            print(json.dumps(a), flush=True)


if __name__ == "__main__":
    main()
