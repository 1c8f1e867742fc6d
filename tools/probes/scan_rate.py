"""Rate of the device prefix scan (zscrc_device_scan) over the 3,355,443
records of a 1 GiB device-resident log image of config 4's record shape (the
image tools/probes/pack_rate.py builds), listed on the device and made into 4
levels as if four files of four ages covered the same keys -- the image holds
every key once, so age is dealt, not read: each level ascends strictly
(CHECK_ORDER says so).  Two sets of levels:
  overlap   every record goes to one level at random, one record in three also
            to a second level, and one in eight of the copies in levels 0 to 2
            is made a delete: the newer copy wins, winning deletes are dropped
  disjoint  every record in exactly one level: nothing superseded, no deletes
Workloads, on each set:
  prefixes_random  distinct prefixes of the list's keys, cut to the longest
                   length at which a prefix has two dozen matches or more (the
                   keys are 16 decimal digits: 14 of them, a hundred matches),
                   at most 65,536 of them, in random order
  prefixes_sorted  the same prefixes in key order
  everything       the one empty prefix: the whole database in order
each at the default table size, at 1 (no table) and at 2,048 splitters,
interleaved in one run, against
  (b) what the call replaces: the lists, the source and the prefixes copied to
      pinned host memory, then zscrc_zs_scan on one core of the same machine;
  (c) context only, for `everything`: zscrc_device_merge of the same lists in
      reverse order with DROP_DELETES, which gives the same rows by a sort.
Every table size's rows are compared with the no-table form's and with the
host scan's.

The timing step runs twice, each a process of its own under its own time
limit; a row holds both runs' medians and their spread.  One JSON line per
workload and table size goes to --out (default profiles/scan/scan_rate.jsonl).
usage (GPU box): python tools/probes/scan_rate.py [--out FILE] [--mib 1024]"""
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

SPLITS = [0, 1, 2048]
WARM, RUNS = 3, 17
NQ = 1 << 16
LEVELS = 4


def prefixes(img, recs, n):
    """(qsrc, queries in random order, queries in key order, prefix length) on the device."""
    import torch
    dev = img.device
    assert bool((recs[:, 1] == 16).all())
    step = 1 << 20
    keys = torch.cat([img[recs[a:a + step, 0][:, None] + torch.arange(16, device=dev)[None, :]]
                      for a in range(0, n, step)])
    for ln in range(15, 0, -1):
        uniq = torch.unique(keys[:, :ln].contiguous(), dim=0)       # in key order
        if n / len(uniq) >= 24:
            break
    nq = min(NQ, len(uniq))
    gen = torch.Generator(device=dev)
    gen.manual_seed(12)
    pick = torch.randperm(len(uniq), generator=gen, device=dev)[:nq]
    q = torch.zeros((nq, 4), dtype=torch.int64, device=dev)
    q[:, 0] = ln * torch.arange(nq, device=dev)
    q[:, 1] = ln
    return (uniq[pick].reshape(-1).contiguous(), uniq[torch.sort(pick).values].reshape(-1).contiguous(), q, ln)


def step_time(args):
    import numpy as np
    import torch
    from zeroskip_amd import repack, zsfile
    img, pairs = build_image(args.mib)
    dev = img.device
    size = img.numel()
    recs, n, _ = listed(img, pairs)
    gen = torch.Generator(device=dev)
    gen.manual_seed(13)
    deal = torch.randint(0, LEVELS, (n,), generator=gen, device=dev)
    also = (deal + 1 + torch.randint(0, LEVELS - 1, (n,), generator=gen, device=dev)) % LEVELS
    also[torch.randint(0, 3, (n,), generator=gen, device=dev) != 0] = -1
    dele = torch.randint(0, 8, (n,), generator=gen, device=dev) == 0
    sets = {"overlap": [], "disjoint": [(recs[deal == l].contiguous(), 0) for l in range(LEVELS)]}
    for l in range(LEVELS):
        r = recs.clone()
        if l < LEVELS - 1:
            r[dele, 2] = zsfile.DELETED
        sets["overlap"].append((r[(deal == l) | (also == l)].contiguous(), 0))
    q_random, q_sorted, q, ln = prefixes(img, recs, n)
    empty = torch.zeros((1, 4), dtype=torch.int64, device=dev)
    work = {"prefixes_random": (q_random, q), "prefixes_sorted": (q_sorted, q), "everything": (img[:0], empty)}
    h_img = img.cpu().numpy()
    rows = []
    for which, name in [(w, n_) for w in sets for n_ in work]:
        levels = sets[which]
        n_total = sum(int(r.shape[0]) for r, _ in levels)
        host_src = (h_img, [(r.cpu().numpy(), b) for r, b in levels])
        qsrc, queries = work[name]
        nq = int(queries.shape[0])
        _, _, _, sized = zsfile.device_scan(img, levels, qsrc, queries, check_order=True, cap=0, cand_cap=n_total)
        r0 = sized.cpu().tolist()
        assert r0[0] in (0, 3) and r0[7] == 0, (name, r0)
        cap, cands = r0[2], r0[3]
        out = {s: (torch.empty((cap, 4), dtype=torch.int64, device=dev),
                   torch.empty(nq + 1, dtype=torch.int64, device=dev),
                   torch.empty(cap, dtype=torch.int64, device=dev),
                   torch.empty(zsfile.SCAN_RES_WORDS, dtype=torch.int64, device=dev)) for s in SPLITS}
        ms = {s: [] for s in SPLITS}
        for it in range(WARM + RUNS):
            for s in SPLITS:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                zsfile.device_scan(img, levels, qsrc, queries, cap=cap, cand_cap=cands, splitters=s, out=out[s])
                e1.record()
                torch.cuda.synchronize()
                if it >= WARM:
                    ms[s].append(e0.elapsed_time(e1))
        res = out[1][3].cpu().tolist()
        assert res[0] == 0 and res[2] == cap and res[3] == cands and res[6] == 0, (name, res)
        assert (res[4] > 0 and res[5] > 0) == (which == "overlap"), (which, res)
        equal = {s: all(bool(torch.equal(a, b)) for a, b in zip(out[s], out[1])) for s in SPLITS}
        assert all(equal.values()), (name, equal)
        merge_ms = None
        if name == "everything":
            mout = torch.empty((n_total, 4), dtype=torch.int64, device=dev)
            mm = []
            for it in range(WARM + RUNS):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _, mres = repack.device_merge(img, levels[::-1], drop_deletes=True, out=mout)
                e1.record()
                torch.cuda.synchronize()
                if it >= WARM:
                    mm.append(e0.elapsed_time(e1))
            assert int(mres[1]) == cap and bool(torch.equal(mout[:cap], out[1][0]))
            merge_ms = round(median(mm), 4)
        # (b) what the call replaces: lists, source and prefixes to the host, one core's scan
        d2h = []
        moved = [r for r, _ in levels] + [img, qsrc, queries]
        pins = [torch.empty(t.shape, dtype=t.dtype).pin_memory() for t in moved]
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for p, t in zip(pins, moved):
                p.copy_(t, non_blocking=True)
            torch.cuda.synchronize()
            d2h.append((time.perf_counter() - t0) * 1e3)
        del pins
        t0 = time.perf_counter()
        hrows, hoffs, hseq, hres = zsfile.scan(host_src[0], host_src[1], qsrc.cpu().numpy(), queries.cpu().numpy(),
                                               cap=cap)
        host_ms = (time.perf_counter() - t0) * 1e3
        same_host = hres.tolist() == res and all(bool(np.array_equal(h, o.cpu().numpy()))
                                                 for h, o in zip((hrows, hoffs, hseq), out[1]))
        assert same_host, name
        for s in SPLITS:
            med = median(ms[s])
            rows.append({"probe": "scan_rate", "image_bytes": size, "records": n, "levels": LEVELS, "level_set": which,
                         "level_records": n_total, "workload": name,
                         "prefixes": nq, "prefix_len": ln if nq > 1 else 0, "candidates": cands, "rows": cap,
                         "splitters": s, "runs": len(ms[s]), "scan_ms_median": round(med, 4),
                         "scan_ms_min": round(min(ms[s]), 4), "scan_ms_max": round(max(ms[s]), 4),
                         "mcandidate_s": round(cands / med / 1e3, 1), "res": res,
                         "scratch_bytes": zsfile.device_scan_scratch_bytes(nq, LEVELS, cands, s),
                         "today": {"d2h_ms": round(median(d2h), 3), "host_scan_ms_one_core": round(host_ms, 3),
                                   "total_ms": round(median(d2h) + host_ms, 3)},
                         "today_over_scan": round((median(d2h) + host_ms) / med, 1),
                         "context": {"device_merge_ms": merge_ms},
                         "equal_to_no_table": equal[s], "equal_to_host": same_host})
    with open(args.tmp, "w") as f:
        json.dump(rows, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan", "scan_rate.jsonl"))
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--step", choices=["time"])
    ap.add_argument("--tmp")
    args = ap.parse_args()
    if args.step:
        return step_time(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__), "--mib", str(args.mib)]
    runs = []
    with tempfile.TemporaryDirectory(prefix="scan_rate_") as work:
        for r in range(2):
            tmp = os.path.join(work, "time%d.json" % r)
            subprocess.run(["timeout", "-k", "10", "500"] + me + ["--step", "time", "--tmp", tmp], check=True)
            runs.append(json.load(open(tmp)))
    with open(args.out, "w") as f:
        for a, b in zip(*runs):
            assert (a["level_set"], a["workload"], a["splitters"]) == (b["level_set"], b["workload"], b["splitters"])
            lo, hi = sorted((a["scan_ms_median"], b["scan_ms_median"]))
            a["scan_ms_median_runs"] = [a["scan_ms_median"], b["scan_ms_median"]]
            a["run_to_run_spread"] = round(hi / lo - 1, 4)
            f.write(json.dumps(a) + "\n")
            print(json.dumps(a), flush=True)


if __name__ == "__main__":
    main()
