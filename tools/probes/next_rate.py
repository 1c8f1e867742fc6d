"""Rate of the device successor stage (zscrc_device_next) over the 3,355,443
records of a 1 GiB device-resident log image of config 4's record shape (the
image tools/probes/pack_rate.py builds), listed on the device and made into 4
overlapping levels as tools/probes/scan_rate.py makes them: every record goes
to one level at random, one record in three also to a second level, and one in
eight of the copies in levels 0 to 2 is made a delete.  The queries are
tools/probes/find_rate.py's: 1 M 16-byte keys, half of them keys of the list,
in random order and in key order.  Workloads:
  page1, page64   the next 1 and the next 64 live keys after every query
  find            zscrc_device_find of the same keys over the same levels in
                  the same run, interleaved with page1: the ratio is what the
                  cursors' merge costs on top of the bisections
  today           what the call replaces: the lists, the source and the keys
                  copied to pinned host memory, then zscrc_zs_next on one core
                  of the same machine (page64: its first 65,536 queries only,
                  and said so in the row)
  paging          the whole database walked from the empty key by chained calls
                  of page 64, the cursor tensor fed back as the query list and
                  one state word read back a round, once; against
                  zscrc_device_scan of the empty prefix in the same run, which
                  gives the same rows in one call
The rows of page1 are compared with the host form's, those of the chain with
the scan's.

The timing step runs twice, each a process of its own under its own time
limit; a row holds both runs' medians and their spread.  One JSON line per
workload goes to --out (default profiles/next/next_rate.jsonl).
usage (GPU box): python tools/probes/next_rate.py [--out FILE] [--mib 1024]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tools.probes.find_rate import batches  # noqa: E402
from tools.probes.pack_rate import build_image, listed, median  # noqa: E402

WARM, RUNS = 3, 17
LEVELS = 4
HOST_PAGE64_NQ = 1 << 16


def once(fn) -> float:
    """One call's milliseconds between two events."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def timed(fn, runs=RUNS):
    return [once(fn) for _ in range(WARM + runs)][WARM:]


def step_time(args):
    import numpy as np
    import torch
    from zeroskip_amd import zsfile
    img, pairs = build_image(args.mib)
    dev = img.device
    recs, n, _ = listed(img, pairs)
    recs = recs.contiguous()
    gen = torch.Generator(device=dev)
    gen.manual_seed(13)
    deal = torch.randint(0, LEVELS, (n,), generator=gen, device=dev)
    also = (deal + 1 + torch.randint(0, LEVELS - 1, (n,), generator=gen, device=dev)) % LEVELS
    also[torch.randint(0, 3, (n,), generator=gen, device=dev) != 0] = -1
    dele = torch.randint(0, 8, (n,), generator=gen, device=dev) == 0
    levels = []
    for l in range(LEVELS):
        r = recs.clone()
        if l < LEVELS - 1:
            r[dele, 2] = zsfile.DELETED
        levels.append((r[(deal == l) | (also == l)].contiguous(), 0))
    n_total = sum(int(r.shape[0]) for r, _ in levels)
    h_img = img.cpu().numpy()
    h_levels = [(r.cpu().numpy(), b) for r, b in levels]
    rows = []
    base = {"probe": "next_rate", "image_bytes": img.numel(), "records": n, "levels": LEVELS, "level_records": n_total}
    work = batches(img, recs, n)
    for name in ("random", "sorted"):
        qsrc, q = work[name]
        nq = int(q.shape[0])
        # the copy the call replaces
        moved = [r for r, _ in levels] + [img, qsrc, q]
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
        h_qsrc, h_q = qsrc.cpu().numpy(), q.cpu().numpy()
        for page in (1, 64):
            out = (torch.empty((nq, page, 4), dtype=torch.int64, device=dev),
                   torch.empty((nq, page), dtype=torch.int64, device=dev),
                   torch.empty((nq, 4), dtype=torch.int64, device=dev),
                   torch.empty(zsfile.NEXT_RES_WORDS, dtype=torch.int64, device=dev))
            fout = (torch.empty((nq, 4), dtype=torch.int64, device=dev), torch.empty(8, dtype=torch.int64, device=dev))
            next_ms, find_ms = [], []
            for it in range(WARM + RUNS):
                next_ms.append(once(lambda: zsfile.device_next(img, levels, qsrc, q, page=page, out=out)))
                find_ms.append(once(lambda: zsfile.device_find(img, levels, qsrc, q, out=fout)))
            next_ms, find_ms = next_ms[WARM:], find_ms[WARM:]
            _, _, _, cres = zsfile.device_next(img, levels, qsrc, q, page=page, check_order=True)
            res = out[3].cpu().tolist()
            assert res[0] == 0 and res[1] == nq and cres.cpu().tolist() == res, (name, page, res)
            assert res[3] == res[2] + res[5] and res[4] > 0 and res[5] > 0, res
            hq = nq if page == 1 else HOST_PAGE64_NQ
            t0 = time.perf_counter()
            hrows, hseq, hcur, hres = zsfile.next_(h_img, h_levels, h_qsrc, h_q[:hq], page=page)
            host_ms = (time.perf_counter() - t0) * 1e3
            same = all(bool(np.array_equal(h, o[:hq].cpu().numpy())) for h, o in zip((hrows, hseq, hcur), out))
            assert same and (hq < nq or hres.tolist() == res), (name, page)
            med, fmed = median(next_ms), median(find_ms)
            rows.append(dict(base, workload="%s_page%d" % (name, page), queries=nq, page=page, runs=len(next_ms),
                             next_ms_median=round(med, 4), next_ms_min=round(min(next_ms), 4),
                             next_ms_max=round(max(next_ms), 4), mquery_s=round(nq / med / 1e3, 1),
                             mrow_s=round(res[2] / med / 1e3, 1), res=res,
                             find_ms_median=round(fmed, 4), find_ms_min=round(min(find_ms), 4),
                             find_ms_max=round(max(find_ms), 4), next_over_find=round(med / fmed, 2),
                             scratch_bytes=zsfile.device_next_scratch_bytes(nq, LEVELS),
                             today={"d2h_ms": round(median(d2h), 3), "host_next_ms_one_core": round(host_ms, 3),
                                    "host_queries": hq,
                                    "total_ms": round(median(d2h) + host_ms, 3) if hq == nq else None},
                             today_over_next=round((median(d2h) + host_ms) / med, 1) if hq == nq else None,
                             equal_to_host=same))
            del out, fout, hrows, hseq, hcur
    # the whole database by chained pages of 64, once, against the scan of the empty prefix
    empty = torch.zeros((1, 4), dtype=torch.int64, device=dev)
    _, _, _, sized = zsfile.device_scan(img, levels, img[:0], empty, cap=0, cand_cap=n_total)
    cap, cands = (int(v) for v in sized[[2, 3]].cpu())
    sout = (torch.empty((cap, 4), dtype=torch.int64, device=dev), torch.empty(2, dtype=torch.int64, device=dev),
            torch.empty(cap, dtype=torch.int64, device=dev),
            torch.empty(zsfile.SCAN_RES_WORDS, dtype=torch.int64, device=dev))
    scan_ms = timed(lambda: zsfile.device_scan(img, levels, img[:0], empty, cap=cap, cand_cap=cands, out=sout))
    page = 64
    got = torch.empty((cap + page, 4), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rws, _, cur, _ = zsfile.device_next(img, levels, img[:0], empty, page=page, inclusive=True)
    at, calls = 0, 0
    while True:
        calls += 1
        got[at:at + page] = rws[0]
        count, state = (int(v) for v in cur[0, 2:].cpu())
        at += count
        if state != zsfile.NEXT_PAGE:
            break
        rws, _, cur, _ = zsfile.device_next(img, levels, img, cur, page=page)
    torch.cuda.synchronize()
    chain_ms = (time.perf_counter() - t0) * 1e3
    assert state == zsfile.NEXT_END and at == cap and bool(torch.equal(got[:cap], sout[0])), (state, at, cap)
    rows.append(dict(base, workload="paging", page=page, rows=cap, calls=calls, runs=1, chain_ms=round(chain_ms, 1),
                     us_per_call=round(chain_ms * 1e3 / calls, 1), scan_runs=len(scan_ms),
                     scan_ms_median=round(median(scan_ms), 4), chain_over_scan=round(chain_ms / median(scan_ms), 1),
                     equal_to_scan=True))
    with open(args.tmp, "w") as f:
        json.dump(rows, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "next", "next_rate.jsonl"))
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--step", choices=["time"])
    ap.add_argument("--tmp")
    args = ap.parse_args()
    if args.step:
        return step_time(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__), "--mib", str(args.mib)]
    runs = []
    with tempfile.TemporaryDirectory(prefix="next_rate_") as work:
        for r in range(2):
            tmp = os.path.join(work, "time%d.json" % r)
            subprocess.run(["timeout", "-k", "10", "500"] + me + ["--step", "time", "--tmp", tmp], check=True)
            runs.append(json.load(open(tmp)))
    with open(args.out, "w") as f:
        for a, b in zip(*runs):
            assert a["workload"] == b["workload"]
            key = "chain_ms" if a["workload"] == "paging" else "next_ms_median"
            lo, hi = sorted((a[key], b[key]))
            a[key + "_runs"] = [a[key], b[key]]
            a["run_to_run_spread"] = round(hi / lo - 1, 4)
            f.write(json.dumps(a) + "\n")
            print(json.dumps(a), flush=True)


if __name__ == "__main__":
    main()
