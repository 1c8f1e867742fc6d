"""Rate of the device value gather (zscrc_device_gather) over the 3,355,443
records of the 1 GiB device-resident log image of tools/probes/find_rate.py.
Three gather lists:
  random  the hits of that probe's 1 M random-order query batch
  sorted  the hits of the same batch in the list's order
  own     the list's own records (a record list is a gather list)
each at tiles 4 KiB, 16 KiB and 64 KiB and with the copy that searches d_offs
in global memory instead of staging it (ZSCRC_GATHER_SEARCH=1), interleaved in
one run, without CRCs; once more at the default tile with CRCs.  Measured in
the same run, what the numbers are compared against:
  (a) a device-to-device copy of as many bytes;
  (b) torch's byte-index gather of the same values (repeat_interleave, arange,
      index), the index build timed too;
  (c) the path the call replaces: hits and source copied to pinned host memory,
      then zscrc_zs_gather on one core.
Every variant's output is compared with the first one's, and with (b)'s and
(c)'s.

Steps, one GPU process at a time, each under its own time limit:
  time   twice, each a process of its own: a row holds both runs' medians and
         their spread
  trace  the same calls, and the device packer over the list, under rocprofv3
         --kernel-trace (a run of its own): each launch alone, and the packer's
         copy launch re-measured beside the gather's
One JSON line per list and variant goes to --out (default
profiles/gather/gather_rate.jsonl).
usage (GPU box): python tools/probes/gather_rate.py [--out FILE] [--mib 1024]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tools.probes.find_rate import batches  # noqa: E402
from tools.probes.pack_rate import UUID, build_image, listed, median  # noqa: E402

VARIANTS = [("tile", 4096), ("tile", 16384), ("tile", 65536), ("search", 0)]
WARM, RUNS = 3, 17
NAMES = ["random", "sorted", "own"]
KERNELS = ["gather_size_kernel", "gather_scan_kernel", "gather_prefix_kernel"]


def label(v):
    return "search" if v[0] == "search" else "tile%d" % v[1]


def gather_lists(img, recs, n):
    """{name: items} on the device: the hits of find_rate's batches, the list itself."""
    from zeroskip_amd import zsfile
    out = {}
    for name, (qsrc, q) in batches(img, recs, n).items():
        if name == "own":
            out[name] = recs
        else:
            hits, res = zsfile.device_find(img, [(recs, 0)], qsrc, q)
            assert int(res[0]) == 0
            out[name] = hits
    return out


def call(zsfile, img, items, bufs, v, crcs=False):
    values, offs, crc, res = bufs
    if v[0] == "search":
        os.environ["ZSCRC_GATHER_SEARCH"] = "1"
    try:
        zsfile.device_gather(img, items, tile_bytes=v[1], out=(values, offs, crc if crcs else None, res))
    finally:
        os.environ.pop("ZSCRC_GATHER_SEARCH", None)


def buffers(torch, zsfile, img, items):
    dev = img.device
    nq = int(items.shape[0])
    _, _, _, res = zsfile.device_gather(img, items, cap=0)
    total = int(res[3])
    return total, (torch.empty(total, dtype=torch.uint8, device=dev), torch.empty(nq + 1, dtype=torch.int64, device=dev),
                   torch.empty(nq, dtype=torch.int32, device=dev), torch.empty(8, dtype=torch.int64, device=dev))


def timed(torch, f, runs=RUNS):
    ms = []
    for it in range(WARM + runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        torch.cuda.synchronize()
        if it >= WARM:
            ms.append(e0.elapsed_time(e1))
    return ms


def step_time(args):
    import numpy as np
    import torch
    from zeroskip_amd import zsfile
    img, pairs = build_image(args.mib)
    dev = img.device
    size = img.numel()
    recs, n, _ = listed(img, pairs)
    recs = recs.contiguous()
    rows = []
    host_img = None
    for name, items in gather_lists(img, recs, n).items():
        nq = int(items.shape[0])
        total, first = buffers(torch, zsfile, img, items)
        bufs = {v: (first if i == 0 else buffers(torch, zsfile, img, items)[1]) for i, v in enumerate(VARIANTS)}
        ms = {v: [] for v in VARIANTS}
        for it in range(WARM + RUNS):
            for v in VARIANTS:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call(zsfile, img, items, bufs[v], v)
                e1.record()
                torch.cuda.synchronize()
                if it >= WARM:
                    ms[v].append(e0.elapsed_time(e1))
        res = first[3].cpu().tolist()
        assert res[0] == 0 and res[1] == nq and res[3] == total, (name, res)
        equal = {v: bool(all(torch.equal(a, b) for a, b in zip(bufs[v][:2] + bufs[v][3:], first[:2] + first[3:])))
                 for v in VARIANTS}
        assert all(equal.values()), (name, equal)
        for v in VARIANTS[1:]:
            bufs[v] = None
        with_crc = timed(torch, lambda: call(zsfile, img, items, first, ("tile", 0), crcs=True))
        # (a) a device-to-device copy of as many bytes
        dst = torch.empty(total, dtype=torch.uint8, device=dev)
        d2d = timed(torch, lambda: dst.copy_(first[0]))
        del dst
        # (b) torch's byte-index gather of the same values
        val = (items[:, 0] >= 0) & (items[:, 2] != -1)          # FIND_NONE and FIND_BAD_QUERY are -1 and -2 as int64
        offs = first[1]

        def index():
            lens = torch.where(val, items[:, 3], torch.zeros_like(items[:, 3]))
            return torch.repeat_interleave(items[:, 2] - offs[:-1], lens, output_size=total) + \
                torch.arange(total, device=dev)

        ix = timed(torch, index, runs=5)
        idx = index()
        tg = timed(torch, lambda: img[idx], runs=5)
        same_torch = bool(torch.equal(img[idx], first[0]))
        del idx
        torch.cuda.empty_cache()
        # (c) the path the call replaces: hits and source to the host, one core's gather
        moved = [items, img]
        pins = [torch.empty(t.shape, dtype=t.dtype).pin_memory() for t in moved]
        d2h = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for p, t in zip(pins, moved):
                p.copy_(t, non_blocking=True)
            torch.cuda.synchronize()
            d2h.append((time.perf_counter() - t0) * 1e3)
        del pins
        if host_img is None:
            host_img = img.cpu().numpy()
        h_items = items.cpu().numpy()
        t0 = time.perf_counter()
        hv, ho, _, hres = zsfile.gather(host_img, h_items, cap=total)
        host_ms = (time.perf_counter() - t0) * 1e3
        same_host = bool(np.array_equal(hv, first[0].cpu().numpy()) and np.array_equal(ho, first[1].cpu().numpy())
                         and hres.tolist() == res)
        assert same_torch and same_host, (name, same_torch, same_host)
        del hv
        for v in VARIANTS:
            med = median(ms[v])
            rows.append({"probe": "gather_rate", "image_bytes": size, "records": n, "list": name, "items": nq,
                         "variant": label(v), "value_bytes": total, "runs": len(ms[v]),
                         "gather_ms_median": round(med, 4), "gather_ms_min": round(min(ms[v]), 4),
                         "gather_ms_max": round(max(ms[v]), 4), "gb_s_out": round(total / med / 1e6, 1), "res": res,
                         "scratch_bytes": zsfile.device_gather_scratch_bytes(nq, v[1]),
                         "default_tile_with_crcs_ms": round(median(with_crc), 4),
                         "d2d_copy_ms": round(median(d2d), 4), "gather_over_d2d": round(med / median(d2d), 2),
                         "torch": {"index_build_ms": round(median(ix), 3), "index_gather_ms": round(median(tg), 3)},
                         "torch_over_gather": round((median(ix) + median(tg)) / med, 1),
                         "today": {"d2h_ms": round(median(d2h), 3), "host_gather_ms_one_core": round(host_ms, 3),
                                   "total_ms": round(median(d2h) + host_ms, 3)},
                         "today_over_gather": round((median(d2h) + host_ms) / med, 1),
                         "equal_to_first_variant": equal[v], "equal_to_torch": same_torch, "equal_to_host": same_host})
    with open(args.tmp, "w") as f:
        json.dump(rows, f)


def step_trace(args):
    import torch
    from zeroskip_amd import repack, zsfile
    img, pairs = build_image(args.mib)
    recs, n, bound = listed(img, pairs)
    recs = recs.contiguous()
    for name, items in gather_lists(img, recs, n).items():
        _, bufs = buffers(torch, zsfile, img, items)
        for v in VARIANTS:
            for _ in range(WARM + RUNS):
                call(zsfile, img, items, bufs, v)
                torch.cuda.synchronize()
        del bufs
    out = torch.empty(bound, dtype=torch.uint8, device=img.device)
    for _ in range(WARM + RUNS):
        repack.device_pack(img, recs, UUID, 1, 1, out=out)
        torch.cuda.synchronize()


def trace_split(tdir):
    """{(list, variant): {launch: median us}} and the packer's copy launch, from step_trace's trace."""
    files = glob.glob(os.path.join(tdir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return None, None
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    per = WARM + RUNS
    # the first launches of each list are the sizing call's (size, scan, prefix): one more of those three per list
    series = {k: [us(r) for r in rows if k in r["Kernel_Name"]] for k in KERNELS}
    copies = [us(r) for r in rows if "gather_copy" in r["Kernel_Name"]]
    if len(copies) != len(NAMES) * len(VARIANTS) * per:
        return None, None
    out = {}
    for li, name in enumerate(NAMES):
        for vi, v in enumerate(VARIANTS):
            at = (li * len(VARIANTS) + vi) * per
            d = {"copy_us": round(median(copies[at + WARM:at + per]), 2)}
            for k in KERNELS:
                s = series[k]
                if len(s) == len(NAMES) * (len(VARIANTS) * per + 1):
                    a2 = li * (len(VARIANTS) * per + 1) + 1 + vi * per
                    d[k.replace("gather_", "").replace("_kernel", "") + "_us"] = round(median(s[a2 + WARM:a2 + per]), 2)
            out[(name, label(v))] = d
    pk = [us(r) for r in rows if "pack_copy_kernel" in r["Kernel_Name"]]
    return out, (round(median(pk[WARM:]), 2) if len(pk) == per else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gather", "gather_rate.jsonl"))
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--step", choices=["time", "trace"])
    ap.add_argument("--tmp")
    args = ap.parse_args()
    if args.step:
        return {"time": step_time, "trace": step_trace}[args.step](args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__), "--mib", str(args.mib)]
    runs = []
    with tempfile.TemporaryDirectory(prefix="gather_rate_") as work:
        for r in range(2):
            tmp = os.path.join(work, "time%d.json" % r)
            subprocess.run(["timeout", "-k", "10", "400"] + me + ["--step", "time", "--tmp", tmp], check=True)
            runs.append(json.load(open(tmp)))
        tdir = os.path.join(work, "trace")
        tr = subprocess.run(["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--output-format", "csv",
                             "-d", tdir, "-o", "run", "--"] + me + ["--step", "trace"])
        if tr.returncode in (124, 134, 137, 139):
            raise SystemExit(f"trace step ended with status {tr.returncode}")
        split, pack_copy = trace_split(tdir) if tr.returncode == 0 else (None, None)
    with open(args.out, "w") as f:
        for a, b in zip(*runs):
            assert (a["list"], a["variant"]) == (b["list"], b["variant"])
            lo, hi = sorted((a["gather_ms_median"], b["gather_ms_median"]))
            a["gather_ms_median_runs"] = [a["gather_ms_median"], b["gather_ms_median"]]
            a["run_to_run_spread"] = round(hi / lo - 1, 4)
            a["launch_us"] = split[(a["list"], a["variant"])] if split else "not measured"
            if a["list"] == "own":
                # the packer writes the same list's keys and headers too: its copy launch's bytes are the region's
                a["pack_copy_launch_us_same_list"] = pack_copy if pack_copy is not None else "not measured"
            f.write(json.dumps(a) + "\n")
            print(json.dumps(a), flush=True)


if __name__ == "__main__":
    main()
