"""Rate of the device packer (zscrc_device_pack) on the records of a 1 GiB
device-resident log image of config 4's record shape (tools/zsdb_gen.py: the
image tools/probes/records_rate.py builds), listed on the device and then
packed, at tile sizes 4 KiB, 16 KiB, 64 KiB and the default, against
  (c) what a caller does today: the image copied to pinned host memory,
      zscrc_zs_records on one core, Packer.add_arrays into a file on a
      memory-backed directory;
  (d) the floor: one device-to-device copy of file_bytes plus
      zscrc_device_span over the same bytes.
The packer's output is compared with (c)'s file byte for byte at full size.

Steps, one GPU process at a time, each under its own time limit:
  time   event-timed packs, the tile sizes interleaved, median of RUNS after
         warm-up; (c) and (d); the comparison
  trace  packs at the default tile under rocprofv3 --kernel-trace (a run of
         its own); then the per-launch times merged in
One JSON line per tile size goes to --out (default profiles/pack/pack_rate.jsonl).
usage (GPU box): python tools/probes/pack_rate.py [--out FILE] [--mib 1024]"""
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

TILES = [4096, 16384, 65536, 0]
WARM, RUNS = 3, 17
KERNELS = ["pack_size_kernel", "pack_scan_kernel", "pack_prefix_kernel", "pack_copy_kernel", "pack_seal_kernel"]
UUID = bytes(range(16))


def build_image(mib: int):
    import torch
    from tools import zsdb_gen as zg
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(4)
    pairs = ((mib << 20) - zg.HDR) // zg.PAIR
    img = zg.log_files(UUID, 0, 1, pairs, 0, False, gen, dev, batched=True).view(-1)
    return img, pairs


def listed(img, pairs):
    """(recs[:n], n, bound) of the image, listed on the device."""
    from zeroskip_amd import repack, zsfile
    recs, res = zsfile.device_records(img, zsfile.ACTIVE, cap=pairs + 8)
    r = res.cpu().tolist()
    assert r[0] == zsfile.END, r
    return recs[:r[1]], r[1], repack.device_pack_bound(r[1], r[4], r[5])


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def step_time(args):
    import numpy as np
    import torch
    from zeroskip_amd import repack
    from zeroskip_amd._lib import check, lib
    img, pairs = build_image(args.mib)
    dev = img.device
    size = img.numel()
    recs, n, bound = listed(img, pairs)
    out = torch.empty(bound, dtype=torch.uint8, device=dev)
    ms = {t: [] for t in TILES}
    for it in range(WARM + RUNS):
        for t in TILES:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _, res = repack.device_pack(img, recs, UUID, 1, 1, out=out, tile_bytes=t)
            e1.record()
            torch.cuda.synchronize()
            if it >= WARM:
                ms[t].append(e0.elapsed_time(e1))
    r = res.cpu().tolist()
    assert r[0] == 0 and r[1] == n, r
    file_bytes = r[2]
    # (c) today's path: D2H, the host lister on one core, the host packer into a memory-backed file
    shm = "/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir()
    path = os.path.join(shm, "pack_rate_%d.zs" % os.getpid())
    pinned = torch.empty(size, dtype=torch.uint8).pin_memory()
    d2h, hl, hp = [], [], []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pinned.copy_(img, non_blocking=True)
        torch.cuda.synchronize()
        d2h.append((time.perf_counter() - t0) * 1e3)
        a = pinned.numpy()
        h = np.empty((pairs + 8, 4), np.uint64)
        cnt = ctypes.c_size_t()
        t0 = time.perf_counter()
        rc = lib().zscrc_zs_records(a.ctypes.data, a.nbytes, 0, h.ctypes.data, len(h), ctypes.byref(cnt))
        hl.append((time.perf_counter() - t0) * 1e3)
        assert rc == 0 and cnt.value == n
        h = h[:n]
        t0 = time.perf_counter()
        with repack.Packer(path, UUID, 1, 1) as p:
            p.add_arrays(a, h[:, 0].copy(), h[:, 1].copy(), a, h[:, 2].copy(), h[:, 3].copy())
        hp.append((time.perf_counter() - t0) * 1e3)
    base = {"d2h_ms": round(median(d2h), 3), "host_records_ms": round(median(hl), 3),
            "host_packer_ms": round(median(hp), 3)}
    base["total_ms"] = round(sum(base.values()), 3)
    want = np.fromfile(path, dtype=np.uint8)
    os.unlink(path)
    assert len(want) == file_bytes
    equal = bool(torch.equal(out[:file_bytes].cpu(), torch.from_numpy(want)))
    assert equal, "the device packer's file differs from the host packer's"
    # (d) the floor: a device-to-device copy of file_bytes and one span CRC over them
    dst = torch.empty(file_bytes, dtype=torch.uint8, device=dev)
    crc = torch.empty(1, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    cp, sp = [], []
    for it in range(WARM + RUNS):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        dst.copy_(out[:file_bytes])
        e[1].record()
        check(lib().zscrc_device_span(dst.data_ptr(), file_bytes, 0, crc.data_ptr(), None, 0, s), "zscrc_device_span")
        e[2].record()
        torch.cuda.synchronize()
        if it >= WARM:
            cp.append(e[0].elapsed_time(e[1]))
            sp.append(e[1].elapsed_time(e[2]))
    floor = {"d2d_copy_ms": round(median(cp), 4), "span_crc_ms": round(median(sp), 4)}
    floor["total_ms"] = round(floor["d2d_copy_ms"] + floor["span_crc_ms"], 4)
    rows = []
    for t in TILES:
        med = median(ms[t])
        rows.append({"probe": "pack_rate", "image_bytes": size, "records": n, "file_bytes": file_bytes,
                     "bound_bytes": bound, "tile_bytes": t, "runs": len(ms[t]), "pack_ms_median": round(med, 4),
                     "pack_ms_min": round(min(ms[t]), 4), "pack_ms_max": round(max(ms[t]), 4),
                     "gb_s_out": round(file_bytes / med / 1e6, 1),
                     "scratch_bytes": repack.device_pack_scratch_bytes(n, t), "today": base,
                     "today_over_pack": round(base["total_ms"] / med, 2), "floor": floor,
                     "pack_over_floor": round(med / floor["total_ms"], 2), "equal_to_host_packer": equal})
    with open(args.tmp, "w") as f:
        json.dump(rows, f)
    print(json.dumps(rows), flush=True)


def step_trace(args):
    import torch
    from zeroskip_amd import repack
    img, pairs = build_image(args.mib)
    recs, n, bound = listed(img, pairs)
    out = torch.empty(bound, dtype=torch.uint8, device=img.device)
    for _ in range(WARM + RUNS):
        repack.device_pack(img, recs, UUID, 1, 1, out=out)
        torch.cuda.synchronize()


def trace_split(tdir):
    """{kernel: median us} of the packer's launches, and the median sum of the
    CRC batch's launches between the copy and the seal, from step_trace's trace."""
    files = glob.glob(os.path.join(tdir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return None
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    out = {}
    for k in KERNELS:
        v = [us(r) for r in rows if k in r["Kernel_Name"]]
        if len(v) != WARM + RUNS:
            return None
        out[k.replace("pack_", "").replace("_kernel", "") + "_us"] = round(median(v[WARM:]), 2)
    batch, cur, inside = [], 0.0, False
    for r in rows:
        if "pack_copy_kernel" in r["Kernel_Name"]:
            cur, inside = 0.0, True
        elif "pack_seal_kernel" in r["Kernel_Name"]:
            batch.append(cur)
            inside = False
        elif inside:
            cur += us(r)
    out["crc_batch_us"] = round(median(batch[WARM:]), 2) if len(batch) == WARM + RUNS else "not measured"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pack", "pack_rate.jsonl"))
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
    with tempfile.TemporaryDirectory(prefix="pack_rate_") as work:
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
            r["launch_us"] = (split or "not measured") if r["tile_bytes"] == 0 else "default tile only"
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
