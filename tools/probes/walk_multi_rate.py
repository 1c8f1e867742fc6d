"""Rate of the many-image device walk (zscrc_device_walk_multi) and of
zscrc_device_verify_images on a device-resident arena of about 1 GiB of
config 4's record shape (tools/zsdb_gen.py: zsbench pairs, one commit per
pair) cut into log files -- 256 files of 4 MiB, and 1,526 files of about
0.67 MiB -- against what a caller does without them: one zscrc_device_walk
(preallocated outputs, library scratch) or one zscrc_device_verify_image per
file, one after another.

Steps, one GPU process at a time, each under its own time limit:
  time   per shape: (a) the multi-walk and (b) the loop of k single walks,
         event-timed, interleaved, median of RUNS after warm-up, their outputs
         compared; (c) verify_images against the loop of verify_image
  trace  the multi-walk alone under rocprofv3 --kernel-trace (a run of its own)
  (then) the trace's per-launch times (table, chain, scan, emit) merged in
One JSON line per shape goes to --out (default profiles/walk/walk_multi_rate.jsonl).
usage (GPU box): python tools/probes/walk_multi_rate.py [--out FILE] [--mib 1024]"""
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

SHAPES = [256, 1526]           # files the arena is cut into
WARM, RUNS = 3, 11
VWARM, VRUNS = 1, 5
KERNELS = ["walk_multi_table_kernel", "walk_multi_chain_kernel", "walk_multi_scan_kernel", "walk_multi_emit_kernel"]


def build_arena(mib: int, files: int):
    """([files, size] uint8 device tensor, pairs per file)."""
    import torch
    from tools import zsdb_gen as zg
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(4)
    pairs = ((mib << 20) // files - zg.HDR) // zg.PAIR
    return zg.log_files(bytes(range(16)), 0, files, pairs, 0, False, gen, dev, batched=True), pairs


def multi_out(k, cap, dev):
    import torch
    from zeroskip_amd import zsfile
    return (torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(cap, dtype=torch.int64, device=dev),
            torch.empty(cap, dtype=torch.int32, device=dev),
            torch.empty((k, zsfile.WALK_ROW_WORDS), dtype=torch.int64, device=dev),
            torch.empty(zsfile.WALK_TOT_WORDS, dtype=torch.int64, device=dev))


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, r


def med(v):
    v = sorted(v)
    return round(v[len(v) // 2], 4)


def step_time(args):
    import torch
    from zeroskip_amd import zsfile
    from zeroskip_amd._lib import lib
    L = lib()
    rows = []
    for files in SHAPES:
        arena, pairs = build_arena(args.mib, files)
        dev, size = arena.device, arena.shape[1]
        flat = arena.view(-1)
        images = [(j * size, size) for j in range(files)]
        per = pairs + 8                                    # room per file; the multi-walk gets the sum
        out = multi_out(files, per * files, dev)
        s_off = torch.empty(per * files, dtype=torch.int64, device=dev)
        s_len = torch.empty(per * files, dtype=torch.int64, device=dev)
        s_res = torch.empty((files, zsfile.WALK_RES_WORDS), dtype=torch.int64, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        base, po, pl, pr = flat.data_ptr(), s_off.data_ptr(), s_len.data_ptr(), s_res.data_ptr()

        def loop_walk():                                   # what a caller does today, without Python's wrapper
            for j in range(files):
                rc = L.zscrc_device_walk(base + j * size, size, po + 8 * per * j, pl + 8 * per * j, per,
                                         pr + 8 * zsfile.WALK_RES_WORDS * j, None, None, 0, stream)
                assert rc == 0, rc

        def multi_walk():
            return zsfile.device_walk_multi(flat, images, cap=per * files, out=out)

        a_ms, b_ms, a_wall, b_wall = [], [], [], []
        for it in range(WARM + RUNS):
            ea, wa, _ = timed(multi_walk)
            eb, wb, _ = timed(loop_walk)
            if it >= WARM:
                a_ms.append(ea), b_ms.append(eb), a_wall.append(wa), b_wall.append(wb)
        # the same spans either way
        off, ln, img, rws, tot = (t.cpu() for t in out)
        res = s_res.cpu()
        n = int(res[0, 1])                                 # commits per file: every file has the same records
        assert 0 < n <= per and torch.equal(res[:, 1], torch.full((files,), n)), res[:, :3]
        assert tot.tolist()[:2] == [0, n * files], tot
        assert torch.equal(rws[:, :3], res[:, :3]), "rows"
        so, sl = s_off.cpu().view(files, per)[:, :n], s_len.cpu().view(files, per)[:, :n]
        assert torch.equal(off[:n * files].view(files, n), so + torch.arange(files)[:, None] * size)
        assert torch.equal(ln[:n * files].view(files, n), sl)
        assert torch.equal(img[:n * files].view(files, n), torch.arange(files, dtype=torch.int32)[:, None]
                           .expand(files, n))

        def loop_verify():
            return [zsfile.verify_device_image(arena[j]) for j in range(files)]

        va, vb = [], []
        for it in range(VWARM + VRUNS):
            _, wa, ra = timed(lambda: zsfile.verify_device_images(flat, images))
            _, wb, rb = timed(loop_verify)
            assert ra == rb and all(r["n_bad"] == 0 and r["n_commits"] == n for r in ra)
            if it >= VWARM:
                va.append(wa), vb.append(wb)
        a, b = med(a_ms), med(b_ms)
        rows.append({"probe": "walk_multi_rate", "files": files, "file_bytes": size, "arena_bytes": size * files,
                     "commits": n * files, "runs": RUNS,
                     "multi_walk_ms": a, "multi_walk_ms_min": round(min(a_ms), 4), "multi_walk_ms_max": round(max(a_ms), 4),
                     "multi_walk_gb_s": round(size * files / a / 1e6, 1), "multi_walk_wall_ms": med(a_wall),
                     "loop_walk_ms": b, "loop_walk_ms_min": round(min(b_ms), 4), "loop_walk_ms_max": round(max(b_ms), 4),
                     "loop_walk_wall_ms": med(b_wall), "loop_over_multi": round(b / a, 2),
                     "verify_runs": VRUNS, "verify_images_wall_ms": med(va), "loop_verify_image_wall_ms": med(vb),
                     "loop_verify_over_verify_images": round(med(vb) / med(va), 2),
                     "scratch_bytes": zsfile.walk_multi_scratch_bytes(images), "equal_to_single_walks": True})
        del arena, flat, out, s_off, s_len
        torch.cuda.empty_cache()
    with open(args.tmp, "w") as f:
        json.dump(rows, f)
    print(json.dumps(rows), flush=True)


def step_trace(args):
    import torch
    from zeroskip_amd import zsfile
    for files in SHAPES:       # not interleaved: the summary cuts the trace by position
        arena, pairs = build_arena(args.mib, files)
        size = arena.shape[1]
        images = [(j * size, size) for j in range(files)]
        out = multi_out(files, (pairs + 8) * files, arena.device)
        for _ in range(WARM + RUNS):
            zsfile.device_walk_multi(arena.view(-1), images, cap=(pairs + 8) * files, out=out)
            torch.cuda.synchronize()
        del arena, out
        torch.cuda.empty_cache()


def trace_split(tdir):
    """{files: {kernel: median us}} from the kernel trace of step_trace."""
    found = glob.glob(os.path.join(tdir, "**", "*kernel_trace.csv"), recursive=True)
    if not found:
        return None
    rows = sorted(csv.DictReader(open(found[0])), key=lambda r: int(r["Start_Timestamp"]))
    per = {k: [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if k in r["Kernel_Name"]]
           for k in KERNELS}
    if any(len(v) != len(SHAPES) * (WARM + RUNS) for v in per.values()):
        return None
    out = {}
    for i, files in enumerate(SHAPES):
        out[files] = {}
        for k, v in per.items():
            runs = sorted(v[i * (WARM + RUNS) + WARM:(i + 1) * (WARM + RUNS)])
            out[files][k.replace("walk_multi_", "").replace("_kernel", "") + "_us"] = round(runs[len(runs) // 2], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "walk", "walk_multi_rate.jsonl"))
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
    with tempfile.TemporaryDirectory(prefix="walk_multi_rate_") as work:
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
            r["launch_us"] = split[r["files"]] if split else "not measured"
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
