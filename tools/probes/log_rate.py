"""Rate of the device log writer (zscrc_device_log) on the records of a 1 GiB
device-resident log image of config 4's record shape (tools/zsdb_gen.py: the
image tools/probes/records_rate.py and pack_rate.py build), listed on the device
and then logged again into a new image, in three shapes -- one transaction a
record, transactions of 64 records, one transaction -- against
  (b) the path it replaces: the list and the source copied to pinned host
      memory, zscrc_zs_log on one core, the image copied back to the device;
  (c) zscrc_device_pack of the same list in the same run, the yardstick of the
      copy launch: the log's bytes are the packer's records region plus one
      commit record a transaction.
The device image is compared with (b)'s byte for byte at full size.

Steps, one GPU process at a time, each under its own time limit:
  time   event-timed calls, the shapes and the packer interleaved, median of
         RUNS after warm-up; (b); the comparison
  trace  the same calls under rocprofv3 --kernel-trace (a run of its own), for
         the two copy launches alone: median, minimum and maximum per output
         byte of log_copy_kernel per shape and of pack_copy_kernel
One JSON line per shape goes to --out (default profiles/devlog/log_rate.jsonl).
usage (GPU box): python tools/probes/log_rate.py [--out FILE] [--mib 1024]"""
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

from tools.probes.pack_rate import UUID, build_image, listed, median  # noqa: E402

SHAPES = ["tx_per_record", "tx_of_64", "one_tx"]
WARM, RUNS = 3, 21
HOST_RUNS = 2


def tables(n, dev):
    import torch
    ends64 = torch.arange(64, n + 64, 64, dtype=torch.int64, device=dev).clamp_(max=n)
    return {"tx_per_record": None, "tx_of_64": ends64,
            "one_tx": torch.tensor([n], dtype=torch.int64, device=dev)}


def prepare(args):
    import torch
    from zeroskip_amd import zsfile
    img, pairs = build_image(args.mib)
    recs, n, pack_bound = listed(img, pairs)
    recs = recs.contiguous()
    tx = tables(n, img.device)
    sums = [int(v) for v in recs[:, [1, 3]].sum(0).cpu()]
    bound = zsfile.device_log_bound(n, n, sums[0], sums[1])
    out = torch.empty(bound, dtype=torch.uint8, device=img.device)
    pout = torch.empty(pack_bound, dtype=torch.uint8, device=img.device)
    return img, recs, n, tx, out, pout


def step_time(args):
    import torch
    from zeroskip_amd import repack, zsfile
    img, recs, n, tx, out, pout = prepare(args)
    ms = {s: [] for s in SHAPES + ["pack"]}
    res = {}
    for it in range(WARM + RUNS):
        for s in SHAPES + ["pack"]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            if s == "pack":
                e0.record()
                _, r = repack.device_pack(img, recs, UUID, 1, 1, out=pout)
                e1.record()
                torch.cuda.synchronize()
                res[s] = r.cpu().tolist()
            else:
                # the wrapper reads the result words back: inside the timed region, as a caller pays it
                e0.record()
                d = zsfile.device_log(img, recs, tx[s], UUID, 1, 1, out=out)
                e1.record()
                torch.cuda.synchronize()
                res[s] = d
            if it >= WARM:
                ms[s].append(e0.elapsed_time(e1))
    assert res["pack"][0] == 0
    # (b) the path it replaces
    hrecs = torch.empty(recs.shape, dtype=torch.int64).pin_memory()
    hsrc = torch.empty(img.numel(), dtype=torch.uint8).pin_memory()
    himg = torch.empty(out.numel(), dtype=torch.uint8).pin_memory()
    back = torch.empty_like(out)
    rows = []
    for s in SHAPES:
        d = res[s]
        assert d["code"] == 0 and d["n"] == n, d["code"]
        end = d["end"]
        d2h, host, h2d = [], [], []
        for _ in range(HOST_RUNS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hrecs.copy_(recs, non_blocking=True)
            hsrc.copy_(img, non_blocking=True)
            torch.cuda.synchronize()
            d2h.append((time.perf_counter() - t0) * 1e3)
            te = None if tx[s] is None else tx[s].cpu().numpy()
            t0 = time.perf_counter()
            h = zsfile.log(hsrc.numpy(), hrecs.numpy(), te, UUID, 1, 1, out=himg.numpy())
            host.append((time.perf_counter() - t0) * 1e3)
            assert h["code"] == 0 and h["end"] == end
            t0 = time.perf_counter()
            back[:end].copy_(himg[:end], non_blocking=True)
            torch.cuda.synchronize()
            h2d.append((time.perf_counter() - t0) * 1e3)
        # out holds another shape's image by now: write this shape's again for the comparison
        d2 = zsfile.device_log(img, recs, tx[s], UUID, 1, 1, out=out)
        equal = d2["end"] == end and bool(torch.equal(back[:end], out[:end]))
        assert equal, "the device image differs from the host twin's (%s)" % s
        med, pmed = median(ms[s]), median(ms["pack"])
        today = {"d2h_ms": round(min(d2h), 3), "host_log_ms": round(min(host), 3), "h2d_ms": round(min(h2d), 3)}
        today["total_ms"] = round(sum(today.values()), 3)
        rows.append({"probe": "log_rate", "shape": s, "image_bytes": img.numel(), "records": n,
                     "commits": d["commits"], "end_bytes": end, "runs": len(ms[s]),
                     "log_ms_median": round(med, 4), "log_ms_min": round(min(ms[s]), 4),
                     "log_ms_max": round(max(ms[s]), 4), "gb_s_out": round(end / med / 1e6, 1),
                     "scratch_bytes": zsfile.device_log_scratch_bytes(n, d["commits"]),
                     "replaced_path": today, "host_runs": HOST_RUNS,
                     "replaced_over_log": round(today["total_ms"] / med, 2),
                     "pack": {"file_bytes": res["pack"][2], "region_bytes": res["pack"][3],
                              "ms_median": round(pmed, 4), "ms_min": round(min(ms["pack"]), 4),
                              "ms_max": round(max(ms["pack"]), 4)},
                     "equal_to_host_twin": equal})
    with open(args.tmp, "w") as f:
        json.dump(rows, f)
    print(json.dumps(rows), flush=True)


def step_trace(args):
    import torch
    from zeroskip_amd import repack, zsfile
    img, recs, n, tx, out, pout = prepare(args)
    for s in SHAPES:
        for _ in range(WARM + RUNS):
            zsfile.device_log(img, recs, tx[s], UUID, 1, 1, out=out)
            torch.cuda.synchronize()
    for _ in range(WARM + RUNS):
        repack.device_pack(img, recs, UUID, 1, 1, out=pout)
        torch.cuda.synchronize()


def trace_split(tdir):
    """{shape | 'pack': [us of the copy launch, the runs after warm-up]} from step_trace's trace."""
    files = glob.glob(os.path.join(tdir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return None
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    lg = [us(r) for r in rows if "log_copy_kernel" in r["Kernel_Name"]]
    pk = [us(r) for r in rows if "pack_copy_kernel" in r["Kernel_Name"]]
    per = WARM + RUNS
    if len(lg) != per * len(SHAPES) or len(pk) != per:
        return None
    out = {s: lg[i * per + WARM:(i + 1) * per] for i, s in enumerate(SHAPES)}
    out["pack"] = pk[WARM:]
    return out


def per_byte(v, nbytes):
    """Median, minimum and maximum of the launch times in picoseconds per output byte, and the median rate."""
    return {"us_median": round(median(v), 2), "ps_per_byte_median": round(median(v) * 1e6 / nbytes, 3),
            "ps_per_byte_min": round(min(v) * 1e6 / nbytes, 3), "ps_per_byte_max": round(max(v) * 1e6 / nbytes, 3),
            "gb_s_median": round(nbytes / median(v) / 1e3, 1), "bytes": nbytes, "runs": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "devlog", "log_rate.jsonl"))
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
    with tempfile.TemporaryDirectory(prefix="log_rate_") as work:
        tmp, tdir = os.path.join(work, "time.json"), os.path.join(work, "trace")
        subprocess.run(["timeout", "-k", "10", "400"] + me + ["--step", "time", "--tmp", tmp], check=True)
        rows = json.load(open(tmp))
        tr = subprocess.run(["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--output-format", "csv",
                             "-d", tdir, "-o", "run", "--"] + me + ["--step", "trace"])
        if tr.returncode in (124, 134, 137, 139):
            raise SystemExit(f"trace step ended with status {tr.returncode}")
        split = trace_split(tdir) if tr.returncode == 0 else None
    with open(args.out, "w") as f:
        for r in rows:
            if split:
                # the log's copy launch writes the records (the packer's region bytes): both per byte of those
                r["copy_launch"] = per_byte(split[r["shape"]], r["pack"]["region_bytes"])
                r["pack_copy_launch"] = per_byte(split["pack"], r["pack"]["region_bytes"])
            else:
                r["copy_launch"] = r["pack_copy_launch"] = "not measured"
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
