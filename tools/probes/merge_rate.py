"""Rate of the device merge (zscrc_device_merge) on the 3,355,443 records of a
1 GiB device-resident log image of config 4's record shape (tools/zsdb_gen.py:
the image tools/probes/pack_rate.py builds), listed on the device, in two
forms -- as listed (the keys ascend) and with the list shuffled -- at
tile_records 256, 512, 1024 and 2048, against
  (b) what a caller does today: the image copied to pinned host memory, then
      the host's sort of the same records -- the merge_s zscrc_zs_repack
      reports for a DB on a memory-backed directory that holds the image as
      its one finalised file, at 16 threads;
  (c) the floor: torch.sort of n_total int64 on the device, a sort that never
      looks at key bytes.
End to end: repack.device_repack of the image against that repack_dir (its
total_s, and with the copy to the host before it); the two files are compared
byte for byte at full size.  The merge's output of both forms is compared with
the model: the image's keys are checked on the host to ascend strictly, so the
winners in key order are the records as listed.

Steps, one GPU process at a time, each under its own time limit:
  time   event-timed merges, the tile sizes interleaved, median of RUNS after
         warm-up; (b), (c), end to end; the comparisons
  trace  merges of the listed form at the default tile under rocprofv3
         --kernel-trace (a run of its own); then the per-launch times merged in
One JSON line per form and tile size goes to --out (default
profiles/merge/merge_rate.jsonl).
usage (GPU box): python tools/probes/merge_rate.py [--out FILE] [--mib 1024]"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tools.probes.pack_rate import UUID, build_image, listed, median  # noqa: E402

TILES = [256, 512, 1024, 2048]
DEFAULT_TILE = 2048  # zscrc_merge.hip's DEF_TILE: what step_trace's calls run at
WARM, RUNS = 3, 17
KERNELS = ["merge_gather_kernel", "merge_sort_kernel", "merge_pass_kernel", "merge_flag_kernel", "merge_scan_kernel",
           "merge_scatter_kernel"]
UUIDSTR = "00010203-0405-0607-0809-0a0b0c0d0e0f"


def forms(recs):
    import torch
    gen = torch.Generator(device=recs.device)
    gen.manual_seed(7)
    perm = torch.randperm(recs.shape[0], generator=gen, device=recs.device)
    return {"listed": recs, "shuffled": recs[perm].contiguous()}


def step_time(args):
    import numpy as np
    import torch
    from zeroskip_amd import repack, zsfile
    from tools import zsdb_gen as zg
    img, pairs = build_image(args.mib)
    dev = img.device
    size = img.numel()
    recs, n, _ = listed(img, pairs)
    recs = recs.contiguous()
    out = torch.empty((n, 4), dtype=torch.int64, device=dev)
    ms, equal = {}, {}
    for form, r in forms(recs).items():
        ms[form] = {t: [] for t in TILES}
        for it in range(WARM + RUNS):
            for t in TILES:
                out.zero_()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _, res = repack.device_merge(img, [(r, 0)], out=out, tile_records=t)
                e1.record()
                torch.cuda.synchronize()
                if it >= WARM:
                    ms[form][t].append(e0.elapsed_time(e1))
                if it == 0:     # every tile size once against the model (the records as listed, checked below)
                    rr = res.cpu().tolist()
                    assert rr[:3] == [0, n, n] and rr[6] == 0 and rr[7] == 0, (form, t, rr)
                    equal[(form, t)] = bool(torch.equal(out, recs))
                    assert equal[(form, t)], "the merge's output differs from the model: %s, tile %d" % (form, t)
    # (c) the floor: a device sort of n int64
    keys = torch.randperm(n, device=dev)
    srt = []
    for it in range(WARM + RUNS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.sort(keys)
        e1.record()
        torch.cuda.synchronize()
        if it >= WARM:
            srt.append(e0.elapsed_time(e1))
    # end to end on the device
    e2e = []
    for it in range(2 + 5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        file_dev, rep = repack.device_repack(img, [(0, size)], [zsfile.FINALISED], UUID, 1, 1, drop_deletes=False)
        torch.cuda.synchronize()
        if it >= 2:
            e2e.append((time.perf_counter() - t0) * 1e3)
    assert rep["records_in"] == n and rep["records_out"] == n, rep
    # (b) today: the image to the host, the host repack of a DB that holds it
    pinned = torch.empty(size, dtype=torch.uint8).pin_memory()
    d2h = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pinned.copy_(img, non_blocking=True)
        torch.cuda.synchronize()
        d2h.append((time.perf_counter() - t0) * 1e3)
    a = pinned.numpy()
    # the model's premise: 16-byte keys that ascend strictly in listed order
    h = recs.cpu().numpy().view(np.uint64)
    assert bool((h[:, 1] == 16).all())
    k = a[(h[:, 0][:, None] + np.arange(16, dtype=np.uint64)[None, :]).astype(np.int64)].view("S16").reshape(-1)
    assert bool((k[1:] > k[:-1]).all()), "the image's keys do not ascend strictly"
    shm = "/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir()
    dbdir = tempfile.mkdtemp(prefix="merge_rate_", dir=shm)
    try:
        host = []
        for _ in range(2):
            for f in os.listdir(dbdir):
                os.unlink(os.path.join(dbdir, f))
            a.tofile(os.path.join(dbdir, "zeroskip-%s-1-1" % UUIDSTR))
            with open(os.path.join(dbdir, ".zsdb"), "wb") as fh:
                fh.write(zg.dotzsdb(4096, UUIDSTR.encode() + b"\0", 2))
            host.append(repack.repack_dir(dbdir, threads=16))
        hrep = min(host, key=lambda r: r["total_s"])
        assert hrep["branch"] == 1 and hrep["records_in"] == n and hrep["records_out"] == n, hrep
        want = np.fromfile(hrep["path"], dtype=np.uint8)
    finally:
        shutil.rmtree(dbdir, ignore_errors=True)
    same_file = len(want) == file_dev.numel() and bool(torch.equal(file_dev.cpu(), torch.from_numpy(want)))
    assert same_file, "device_repack's file differs from the host repack's"
    today = {"d2h_ms": round(median(d2h), 3), "host_merge_ms": round(hrep["merge_s"] * 1e3, 3), "threads": 16}
    today["total_ms"] = round(today["d2h_ms"] + today["host_merge_ms"], 3)
    end = {"device_repack_ms": round(median(e2e), 3), "repack_dir_ms": round(hrep["total_s"] * 1e3, 3),
           "repack_dir_list_ms": round(hrep["list_s"] * 1e3, 3), "repack_dir_write_ms": round(hrep["write_s"] * 1e3, 3),
           "d2h_ms": today["d2h_ms"], "file_bytes": int(len(want)), "equal_to_host_repack_file": same_file}
    end["repack_dir_over_device_repack"] = round(end["repack_dir_ms"] / end["device_repack_ms"], 2)
    floor = {"torch_sort_int64_ms": round(median(srt), 4)}
    rows = []
    for form in ms:
        for t in TILES:
            med = median(ms[form][t])
            rows.append({"probe": "merge_rate", "image_bytes": size, "records": n, "form": form, "tile_records": t,
                         "runs": len(ms[form][t]), "merge_ms_median": round(med, 4),
                         "merge_ms_min": round(min(ms[form][t]), 4), "merge_ms_max": round(max(ms[form][t]), 4),
                         "mrec_s": round(n / med / 1e3, 1), "scratch_bytes": repack.device_merge_scratch_bytes(n, t),
                         "today": today, "today_over_merge": round(today["total_ms"] / med, 2), "floor": floor,
                         "merge_over_floor": round(med / floor["torch_sort_int64_ms"], 2),
                         "equal_to_model": equal[(form, t)], "end_to_end": end})
    with open(args.tmp, "w") as f:
        json.dump(rows, f)
    print(json.dumps(rows), flush=True)


def step_trace(args):
    import torch
    from zeroskip_amd import repack
    img, pairs = build_image(args.mib)
    recs, n, _ = listed(img, pairs)
    out = torch.empty((n, 4), dtype=torch.int64, device=img.device)
    for _ in range(WARM + RUNS):
        repack.device_merge(img, [(recs, 0)], out=out)
        torch.cuda.synchronize()


def trace_split(tdir):
    """{kernel: median us per call} of the merge's launches (the passes of a call summed), from step_trace's trace."""
    files = glob.glob(os.path.join(tdir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return None
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    calls = []
    for r in rows:
        name = next((k for k in KERNELS if k in r["Kernel_Name"]), None)
        if name is None:
            continue
        if name == KERNELS[0]:
            calls.append(dict.fromkeys(KERNELS, 0.0))
            calls[-1]["passes"] = 0
        if calls:
            calls[-1][name] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            calls[-1]["passes"] += name == "merge_pass_kernel"
    if len(calls) != WARM + RUNS:
        return None
    out = {k.replace("merge_", "").replace("_kernel", "") + "_us": round(median([c[k] for c in calls[WARM:]]), 2)
           for k in KERNELS}
    out["passes"] = calls[-1]["passes"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge", "merge_rate.jsonl"))
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
    with tempfile.TemporaryDirectory(prefix="merge_rate_") as work:
        tmp, tdir = os.path.join(work, "time.json"), os.path.join(work, "trace")
        subprocess.run(["timeout", "-k", "10", "420"] + me + ["--step", "time", "--tmp", tmp], check=True)
        rows = json.load(open(tmp))
        tr = subprocess.run(["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--output-format", "csv",
                             "-d", tdir, "-o", "run", "--"] + me + ["--step", "trace"])
        if tr.returncode in (124, 134, 137, 139):
            raise SystemExit(f"trace step ended with status {tr.returncode}")
        split = trace_split(tdir) if tr.returncode == 0 else None
    with open(args.out, "w") as f:
        for r in rows:
            r["launch_us"] = (split or "not measured") if (r["tile_records"], r["form"]) == (DEFAULT_TILE, "listed") \
                else "default tile, listed form only"
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
