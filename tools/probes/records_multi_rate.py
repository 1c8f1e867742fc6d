"""Rate of the many-image record lister (zscrc_device_records_multi) on a
device-resident arena of about 1 GiB of config 4's record shape
(tools/zsdb_gen.py: zsbench pairs, one commit per pair) cut into log files --
256 files of 4 MiB, and 1,526 files of about 0.67 MiB -- against
  - what a caller did without it: one zscrc_device_records per file
    (preallocated outputs, library scratch), one after another;
  - zscrc_device_walk_multi on the same arena (the one call adds 32-byte
    entries to what the walk writes), beside the same ratio for one image of
    the arena's size (zscrc_device_records against zscrc_device_walk);
and of repack.device_repack over the 1,526-file arena end to end against the
same repack listing per file (what device_repack did before the one call).

Steps, each a fresh process under its own time limit, one at a time:
  time    per shape: the one call, the loop and the many-image walk,
          event-timed, interleaved, median of RUNS after warm-up, the outputs
          of the first two compared
  single  one image: zscrc_device_records and zscrc_device_walk, the same way
  repack  device_repack both ways, wall clock, the files compared
  trace   the one call alone under rocprofv3 --kernel-trace (a run of its own)
  (then)  the trace's per-launch times (table, chain, scan, emit) merged in
One JSON line per shape goes to --out (default
profiles/records_multi/records_multi_rate.jsonl).
usage (GPU box): python tools/probes/records_multi_rate.py [--out FILE] [--mib 1024]"""
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
REPACK_FILES = 1526
WARM, RUNS = 3, 11
PWARM, PRUNS = 1, 5
KERNELS = ["records_multi_table_kernel", "records_multi_chain_kernel", "records_multi_scan_kernel",
           "records_multi_emit_kernel"]


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
    return (torch.empty((cap, 4), dtype=torch.int64, device=dev),
            torch.empty((k, zsfile.RECORDS_ROW_WORDS), dtype=torch.int64, device=dev),
            torch.empty(zsfile.RECORDS_TOT_WORDS, dtype=torch.int64, device=dev))


def walk_out(k, cap, dev):
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


def spread(v):
    return {"min": round(min(v), 4), "max": round(max(v), 4)}


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
        per = pairs + 8                                    # room per file; the one call gets the sum
        out = multi_out(files, per * files, dev)
        wout = walk_out(files, per * files, dev)
        s_recs = torch.empty((per * files, 4), dtype=torch.int64, device=dev)
        s_res = torch.empty((files, zsfile.RECORDS_RES_WORDS), dtype=torch.int64, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        base, pr, ps = flat.data_ptr(), s_recs.data_ptr(), s_res.data_ptr()

        def loop_records():                                # what a caller did before, without Python's wrapper
            for j in range(files):
                rc = L.zscrc_device_records(base + j * size, size, zsfile.ACTIVE, pr + 32 * per * j, per,
                                            ps + 8 * zsfile.RECORDS_RES_WORDS * j, None, None, 0, stream)
                assert rc == 0, rc

        def multi_records():
            return zsfile.device_records_multi(flat, images, cap=per * files, out=out)

        def multi_walk():
            return zsfile.device_walk_multi(flat, images, cap=per * files, out=wout)

        a_ms, b_ms, w_ms, a_wall, b_wall = [], [], [], [], []
        for it in range(WARM + RUNS):
            ea, wa, _ = timed(multi_records)
            eb, wb, _ = timed(loop_records)
            ew, _, _ = timed(multi_walk)
            if it >= WARM:
                a_ms.append(ea), b_ms.append(eb), w_ms.append(ew), a_wall.append(wa), b_wall.append(wb)
        # the same records either way
        recs, rws, tot = (t.cpu() for t in out)
        res = s_res.cpu()
        n = int(res[0, 1])                                 # records per file: every file has the same shape
        assert 0 < n <= per and torch.equal(res[:, 1], torch.full((files,), n)), res[:, :3]
        assert tot.tolist()[:2] == [0, n * files] and int(tot[7]) == 0, tot
        assert torch.equal(rws[:, :9], res[:, :9]), "rows"
        assert tot.tolist()[2:5] == res[:, 3:6].sum(0).tolist() and tot.tolist()[5:7] == res[:, 6:8].max(0)[0].tolist()
        want = s_recs.cpu().view(files, per, 4)[:, :n].clone()
        add = (torch.arange(files) * size)[:, None]
        want[:, :, 0] += add
        want[:, :, 2] += add * (want[:, :, 2] != zsfile.DELETED)
        assert torch.equal(recs[:n * files].view(files, n, 4), want)
        a, b, w = med(a_ms), med(b_ms), med(w_ms)
        rows.append({"probe": "records_multi_rate", "files": files, "file_bytes": size, "arena_bytes": size * files,
                     "records": n * files, "record_bytes_out": 32 * n * files, "runs": RUNS,
                     "multi_records_ms": a, "multi_records_ms_spread": spread(a_ms),
                     "multi_records_gb_s": round(size * files / a / 1e6, 1), "multi_records_wall_ms": med(a_wall),
                     "loop_records_ms": b, "loop_records_ms_spread": spread(b_ms), "loop_records_wall_ms": med(b_wall),
                     "loop_over_multi": round(b / a, 2),
                     "multi_walk_ms": w, "multi_walk_ms_spread": spread(w_ms), "records_over_walk": round(a / w, 3),
                     "scratch_bytes": zsfile.records_multi_scratch_bytes(images), "equal_to_single_listers": True})
        del arena, flat, out, wout, s_recs
        torch.cuda.empty_cache()
    with open(args.tmp, "w") as f:
        json.dump(rows, f)
    print(json.dumps(rows), flush=True)


def step_single(args):
    import torch
    from zeroskip_amd import zsfile
    arena, pairs = build_arena(args.mib, 1)
    img, cap = arena.view(-1), pairs + 8
    dev = img.device
    rout = (torch.empty((cap, 4), dtype=torch.int64, device=dev),
            torch.empty(zsfile.RECORDS_RES_WORDS, dtype=torch.int64, device=dev))
    wout = (torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(cap, dtype=torch.int64, device=dev),
            torch.empty(zsfile.WALK_RES_WORDS, dtype=torch.int64, device=dev))
    r_ms, w_ms = [], []
    for it in range(WARM + RUNS):
        er, _, _ = timed(lambda: zsfile.device_records(img, zsfile.ACTIVE, cap=cap, out=rout))
        ew, _, _ = timed(lambda: zsfile.device_walk(img, cap=cap, out=wout))
        if it >= WARM:
            r_ms.append(er), w_ms.append(ew)
    r, w = rout[1].cpu().tolist(), wout[2].cpu().tolist()
    assert r[0] == zsfile.END and w[0] == zsfile.END and r[1] > 0 and w[1] > 0, (r, w)
    row = {"image_bytes": img.numel(), "records": r[1], "commits": w[1], "records_ms": med(r_ms), "records_ms_spread": spread(r_ms),
           "walk_ms": med(w_ms), "walk_ms_spread": spread(w_ms), "records_over_walk": round(med(r_ms) / med(w_ms), 3)}
    with open(args.tmp, "w") as f:
        json.dump(row, f)
    print(json.dumps(row), flush=True)


def per_file_repack(d_arena, images, uuid, startidx, endidx):
    """repack.device_repack as it listed before the one call: zscrc_device_records
    and one read of the result words per file."""
    import torch
    from zeroskip_amd import repack, zsfile
    lists = []
    for off, size in images:
        recs, res = zsfile.device_records(d_arena[off:off + size], zsfile.FINALISED)
        code, n = (int(v) for v in res[:2].cpu())
        assert code == zsfile.END, (off, code)
        lists.append((recs[:n], off))
    n_in = sum(int(r.shape[0]) for r, _ in lists)
    merged, mres = repack.device_merge(d_arena, lists, out=torch.empty((n_in, 4), dtype=torch.int64,
                                                                       device=d_arena.device))
    m = [int(v) for v in mres.cpu()]
    assert m[0] == 0, m
    image, pres = repack.device_pack(d_arena, merged[:m[1]], uuid, startidx, endidx)
    return image, [int(v) for v in pres.cpu()]


def step_repack(args):
    import torch
    from zeroskip_amd import repack, zsfile
    files = REPACK_FILES
    arena, pairs = build_arena(args.mib, files)
    size, flat = arena.shape[1], arena.view(-1)
    images = [(j * size, size) for j in range(files)]
    uuid = bytes(range(16))
    one, loop = [], []
    for it in range(PWARM + PRUNS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        img_a, rep = repack.device_repack(flat, images, [zsfile.FINALISED] * files, uuid, 0, files - 1, False)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        img_b, p = per_file_repack(flat, images, uuid, 0, files - 1)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        assert rep["records_in"] > 0 and p == rep["pack"] and torch.equal(img_a, img_b)
        if it >= PWARM:
            one.append((t1 - t0) * 1e3), loop.append((t2 - t1) * 1e3)
        del img_a, img_b
    row = {"files": files, "arena_bytes": size * files, "records_in": rep["records_in"],
           "records_out": rep["records_out"], "file_bytes": rep["file_bytes"], "runs": PRUNS,
           "device_repack_wall_ms": med(one), "device_repack_wall_ms_spread": spread(one),
           "per_file_listing_wall_ms": med(loop), "per_file_listing_wall_ms_spread": spread(loop),
           "per_file_over_one_call": round(med(loop) / med(one), 2), "files_equal": True}
    with open(args.tmp, "w") as f:
        json.dump(row, f)
    print(json.dumps(row), flush=True)


def step_trace(args):
    import torch
    from zeroskip_amd import zsfile
    for files in SHAPES:       # not interleaved: the summary cuts the trace by position
        arena, pairs = build_arena(args.mib, files)
        size = arena.shape[1]
        images = [(j * size, size) for j in range(files)]
        out = multi_out(files, (pairs + 8) * files, arena.device)
        for _ in range(WARM + RUNS):
            zsfile.device_records_multi(arena.view(-1), images, cap=(pairs + 8) * files, out=out)
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
            out[files][k.replace("records_multi_", "").replace("_kernel", "") + "_us"] = round(runs[len(runs) // 2], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "records_multi", "records_multi_rate.jsonl"))
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--step", choices=["time", "single", "repack", "trace"])
    ap.add_argument("--tmp")
    args = ap.parse_args()
    if args.step:
        return {"time": step_time, "single": step_single, "repack": step_repack, "trace": step_trace}[args.step](args)
    odir = os.path.dirname(os.path.abspath(args.out))
    os.makedirs(odir, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__), "--mib", str(args.mib)]
    # intermediate files and the raw trace stay out of the results' directory
    with tempfile.TemporaryDirectory(prefix="records_multi_rate_") as work:
        got = {}
        for step, limit in (("time", 400), ("single", 200), ("repack", 400)):
            tmp = os.path.join(work, step + ".json")
            subprocess.run(["timeout", "-k", "10", str(limit)] + me + ["--step", step, "--tmp", tmp], check=True)
            got[step] = json.load(open(tmp))
        tdir = os.path.join(work, "trace")
        tr = subprocess.run(["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--output-format", "csv",
                             "-d", tdir, "-o", "run", "--"] + me + ["--step", "trace"])
        if tr.returncode in (124, 134, 137, 139):
            raise SystemExit(f"trace step ended with status {tr.returncode}")
        split = trace_split(tdir) if tr.returncode == 0 else None
    with open(args.out, "w") as f:
        for r in got["time"]:
            r["single_image"] = got["single"]
            if r["files"] == REPACK_FILES:
                r["device_repack"] = got["repack"]
            r["launch_us"] = split[r["files"]] if split else "not measured"
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
