"""Rate of the device record lister (zscrc_device_records) on a 1 GiB
device-resident log image of config 4's record shape (tools/zsdb_gen.py:
zsbench pairs, one commit per pair), at block sizes 256 KiB, 1 MiB and 4 MiB,
against what a caller had to do before it existed: copy the image to pinned
host memory and run zscrc_zs_records on one core.

Steps, one GPU process at a time, each under its own time limit:
  time   event-timed listings, the block sizes interleaved, median of RUNS
         after warm-up; the baseline; the results compared with the host lister
  trace  the same listings under rocprofv3 --kernel-trace (a run of its own)
  (then) the trace's per-launch times (table, chain, emit) merged in
One JSON line per block size goes to --out (default profiles/walk/records_rate.jsonl).
usage (GPU box): python tools/probes/records_rate.py [--out FILE] [--mib 1024]"""
import argparse
import csv
import ctypes
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

BLOCKS = [256 << 10, 1 << 20, 4 << 20]
WARM, RUNS = 3, 17
KERNELS = ["records_table_kernel", "records_chain_kernel", "records_emit_kernel"]


def build_image(mib: int):
    import torch
    from tools import zsdb_gen as zg
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(4)
    pairs = ((mib << 20) - zg.HDR) // zg.PAIR
    img = zg.log_files(bytes(range(16)), 0, 1, pairs, 0, False, gen, dev, batched=True).view(-1)
    return img, pairs


def host_records(a, cap):
    import numpy as np
    from zeroskip_amd._lib import lib
    recs = np.empty((cap, 4), np.uint64)
    n = ctypes.c_size_t()
    t0 = time.perf_counter()
    rc = lib().zscrc_zs_records(a.ctypes.data, a.nbytes, 0, recs.ctypes.data, cap, ctypes.byref(n))
    return (time.perf_counter() - t0) * 1e3, rc, n.value, recs


def step_time(args):
    import numpy as np
    import torch
    from zeroskip_amd import zsfile
    img, pairs = build_image(args.mib)
    dev = img.device
    size, cap = img.numel(), pairs + 8
    out = (torch.empty((cap, 4), dtype=torch.int64, device=dev),
           torch.empty(zsfile.RECORDS_RES_WORDS, dtype=torch.int64, device=dev))
    # the baseline: D2H into pinned memory, then the host lister on one core
    pinned = torch.empty(size, dtype=torch.uint8).pin_memory()
    d2h, hl = [], []
    for _ in range(6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pinned.copy_(img, non_blocking=True)
        torch.cuda.synchronize()
        d2h.append((time.perf_counter() - t0) * 1e3)
        ms, hrc, hn, hrecs = host_records(pinned.numpy(), cap)
        hl.append(ms)
    d2h, hl = d2h[1:], hl[1:]
    base = {"d2h_ms": round(float(np.median(d2h)), 3), "host_records_ms": round(float(np.median(hl)), 3)}
    base["total_ms"] = round(base["d2h_ms"] + base["host_records_ms"], 3)
    h = hrecs[:hn]
    want = torch.from_numpy(h.view(np.int64)).to(dev)
    folds = [int((h[:, 2] == np.uint64(2**64 - 1)).sum()), int(h[:, 1].sum(dtype=np.uint64)),
             int(h[:, 3].sum(dtype=np.uint64)), int(h[:, 1].max()), int(h[:, 3].max())]
    ms = {b: [] for b in BLOCKS}
    for it in range(WARM + RUNS):
        for b in BLOCKS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            recs, res = zsfile.device_records(img, zsfile.ACTIVE, cap=cap, block_bytes=b, out=out)
            e1.record()
            torch.cuda.synchronize()
            if it >= WARM:
                ms[b].append(e0.elapsed_time(e1))
            if it in (0, WARM + RUNS - 1):
                r = res.cpu().tolist()
                assert r[:3] == [hrc, hn, size] and r[8] == -1, (b, r)
                assert r[3:8] == folds, (b, r, folds)
                assert torch.equal(recs[:hn], want), b
    rows = []
    for b in BLOCKS:
        med = float(np.median(ms[b]))
        rows.append({"probe": "records_rate", "image_bytes": size, "records": hn, "record_bytes_out": hn * 32,
                     "block_bytes": b, "tile_bytes": 16384, "runs": len(ms[b]), "records_ms_median": round(med, 4),
                     "records_ms_min": round(min(ms[b]), 4), "records_ms_max": round(max(ms[b]), 4),
                     "gb_s": round(size / med / 1e6, 1),
                     "scratch_bytes": zsfile.records_scratch_bytes(size, zsfile.ACTIVE, b), "baseline": base,
                     "baseline_over_records": round(base["total_ms"] / med, 2), "equal_to_host_lister": True})
    with open(args.tmp, "w") as f:
        json.dump(rows, f)
    print(json.dumps(rows), flush=True)


def step_trace(args):
    import torch
    from zeroskip_amd import zsfile
    img, pairs = build_image(args.mib)
    cap = pairs + 8
    out = (torch.empty((cap, 4), dtype=torch.int64, device=img.device),
           torch.empty(zsfile.RECORDS_RES_WORDS, dtype=torch.int64, device=img.device))
    for b in BLOCKS:           # not interleaved: the summary cuts the trace by position
        for _ in range(WARM + RUNS):
            zsfile.device_records(img, zsfile.ACTIVE, cap=cap, block_bytes=b, out=out)
            torch.cuda.synchronize()


def trace_split(tdir):
    """{block_bytes: {kernel: median us}} from the kernel trace of step_trace."""
    files = glob.glob(os.path.join(tdir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return None
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    per = {k: [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if k in r["Kernel_Name"]]
           for k in KERNELS}
    if any(len(v) != len(BLOCKS) * (WARM + RUNS) for v in per.values()):
        return None
    out = {}
    for i, b in enumerate(BLOCKS):
        out[b] = {}
        for k, v in per.items():
            runs = sorted(v[i * (WARM + RUNS) + WARM:(i + 1) * (WARM + RUNS)])
            out[b][k.replace("records_", "").replace("_kernel", "") + "_us"] = round(runs[len(runs) // 2], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "walk", "records_rate.jsonl"))
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--step", choices=["time", "trace"])
    ap.add_argument("--tmp")
    args = ap.parse_args()
    if args.step:
        return {"time": step_time, "trace": step_trace}[args.step](args)
    odir = os.path.dirname(os.path.abspath(args.out))
    os.makedirs(odir, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__), "--mib", str(args.mib)]
    # intermediate files and the raw trace stay out of the results' directory
    with tempfile.TemporaryDirectory(prefix="records_rate_") as work:
        tmp, tdir = os.path.join(work, "time.json"), os.path.join(work, "trace")
        subprocess.run(["timeout", "-k", "10", "300"] + me + ["--step", "time", "--tmp", tmp], check=True)
        rows = json.load(open(tmp))
        tr = subprocess.run(["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--output-format", "csv",
                             "-d", tdir, "-o", "run", "--"] + me + ["--step", "trace"])
        if tr.returncode in (124, 134, 137, 139):
            raise SystemExit(f"trace step ended with status {tr.returncode}")
        split = trace_split(tdir) if tr.returncode == 0 else None
    with open(args.out, "w") as f:
        for r in rows:
            r["launch_us"] = split[r["block_bytes"]] if split else "not measured"
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
