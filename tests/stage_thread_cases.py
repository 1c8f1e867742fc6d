"""Inputs and expected values for the device stages called from several host
threads at once (tests/test_stage_thread_cases.py on the CPU,
tests/test_gpu_stage_threads.py on the GPU): one object per thread, built from
the stages' own case modules and their references -- the format oracle's
FileWriter and walk (oracle/zs_format.py), the Python models of
tests/merge_cases.py and tests/pack_cases.py, and the host twins zscrc_zs_walk,
_records, _find, _gather, _scan, _next and _log.  No device code is a reference
and no GPU is needed.  The builders of tests/gather_cases.py, scan_cases.py,
next_cases.py and log_cases.py make small cases of fixed content, each with its
own source; here the four stages read one source of equal shape per thread, so
the queries, prefixes and the transaction table are laid out here (with
find_cases.lay_queries, as those modules do) and the expected words come from
the host twins those modules' own tests hold against their Python models.

All NT threads have the same shapes -- record counts, list lengths, caps, image
and source sizes, and therefore the same value of every *_scratch_bytes
function -- and other bytes: thread t has a key tag and value bytes of its own
and lays its records, queries, prefixes and transactions out in an order of its
own, so that every expected output (offsets included) differs between any two
threads.  A call that read another thread's scratch, staging or list cannot
give the expected words by accident.

Sizes (shape()), the smallest at which no stage is a single short launch:
  levels        3 sorted lists of 10,000 records each over one source of
                2.06 MB, 16-byte keys from 20,000 ids (about half of a level's
                keys are in each other level), values of 0 .. 120 bytes; one
                record in five of the newest level and one in seven of the
                middle one is a delete, few of the oldest
  merge / pack  30,000 records in, 17,521 winners (2,778 deletes among them,
                12,479 records superseded), a packed file of 2.01 MB; the same
                list logged in 3,523 transactions of 2 .. 8 records, 1.90 MB
  queries       4,096 keys for find and next (half present, 323 deleted; page 1
                and 8), 48 prefixes for scan (15,059 candidates, 7,317 rows)
  active image  10,000 records in 3,372 transactions, 1.46 MB: 179 walk blocks
                of 8,192 bytes (tile 1,024)
  arena         that image, a finalised one of 8,000 records (1.18 MB, its last
                commit the stale finalise commit) and an active one of 1,200
                with one corrupted commit, at offsets 3, 1 and 2 mod 8: 2.82 MB,
                so that the many-image calls need more library scratch (2.83 MB)
                than the merge (2.67 MB), the largest of the others
  hashing       the variable batch of tests/test_gpu_threads.py (3,000 records,
                12.6 MB) and a span of 3 MiB + 7
Measured on an MI355X at rest (medians of 9): one pass of a thread takes 5.4 ms
of device time -- group A 3.9 ms (zscrc_device_verify_images allocates, waits
for its stream and frees several times), B 0.67 ms, C 0.56 ms, D 0.18 ms; one
call: merge 0.32 ms, walk_multi 0.19, records 0.18, pack 0.17, scan 0.17, log
0.16, next (page 8) 0.14, gather 0.10, find 0.06 ms.  Building the four cases takes 1.0 s there."""
import ctypes
import functools

import numpy as np

from oracle import oracle
from oracle import zs_format as zf
from tests import find_cases as fc
from tests import merge_cases as mc
from tests import pack_cases as pc
from tests import records_images as ri
from tests import walk_images as wi
from tests.images import U64_MAX
from zeroskip_amd import repack, zsfile
from zeroskip_amd._lib import lib

NT = 4
WALK_BLOCK, WALK_TILE = 8192, 1024
IDS, LEVEL_N, K = 20000, 10000, 3
NQ, PAGES = 4096, (1, 8)
N_PREFIX = 48
SCAN_CAP, CAND_CAP = 16384, 32768       # rows and candidates the scan's buffers hold
GATHER_CAP = 1 << 18                    # bytes the gather's buffer holds
ACTIVE_N, FINAL_N, SMALL_N = 10000, 8000, 1200
GAPS = (3, 6, 9)                        # bytes before each image of the arena
BAD_COMMIT = 40                         # thread t's small image: commit 40 + t is corrupted
SPAN_LEN, SPAN_OFF = (3 << 20) + 7, 3
BATCH_N = 3000
UUID = bytes(range(32, 48))
STARTIDX, ENDIDX = 2, 7


class Shape:
    """What every thread shares: which ids a level holds, which records are
    deletes, every length, the queries' ids, the images' schedules."""

    def __init__(self):
        rng = np.random.default_rng(7)
        self.level_ids = [np.sort(rng.choice(IDS, LEVEL_N, replace=False)) for _ in range(K)]
        self.level_del = [rng.random(LEVEL_N) < p for p in (0.2, 0.14, 0.03)]
        self.level_vlen = [rng.integers(0, 121, LEVEL_N) for _ in range(K)]
        present = np.unique(np.concatenate(self.level_ids))
        absent = np.setdiff1d(np.arange(IDS + NQ), present)
        assert len(absent) >= NQ // 2
        self.n_out = len(present)                         # the merge's winners
        self.query_ids = np.concatenate([rng.choice(present, NQ // 2, replace=False),
                                         rng.choice(absent, NQ // 2, replace=False)])
        # prefixes as (digits of the id kept, id): 40 blocks of 100 ids, 6 of 1,000, 2 that match nothing
        self.prefixes = [(9, int(i)) for i in rng.choice(IDS // 100, 40, replace=False) * 100] + \
                        [(8, int(i)) for i in rng.choice(IDS // 1000, 6, replace=False) * 1000] + \
                        [(9, 10 * IDS), (11, int(absent[0]))]
        assert len(self.prefixes) == N_PREFIX
        # the log's transactions: sizes of 2 .. 8 records that sum to n_out
        sizes = []
        while sum(sizes) < self.n_out:
            sizes.append(min(int(rng.integers(2, 9)), self.n_out - sum(sizes)))
        self.tx_sizes = sizes
        self.images = [self._schedule(rng, n) for n in (ACTIVE_N, FINAL_N, SMALL_N)]
        # the hashing batch of tests/test_gpu_threads.py
        lens = np.random.default_rng(21).integers(0, 3000, BATCH_N).astype(np.uint64)
        lens[:3] = [5 << 20, 3 << 20, 70000]
        offs = np.zeros(BATCH_N, np.uint64)
        offs[1:] = np.cumsum(lens[:-1])
        self.b_offs, self.b_lens = offs, lens
        self.b_bytes = int(offs[-1] + lens[-1])
        assert self.b_bytes >= SPAN_OFF + SPAN_LEN

    @staticmethod
    def _schedule(rng, n):
        """(records as (id, value length or -1 for a delete), transaction sizes)."""
        ids = rng.integers(0, IDS, n)
        vlen = np.where(rng.random(n) < 0.125, -1, rng.integers(0, 201, n))
        sizes = []
        while sum(sizes) < n:
            sizes.append(min(int(rng.integers(1, 6)), n - sum(sizes)))
        return list(zip(ids.tolist(), vlen.tolist())), sizes


@functools.lru_cache(maxsize=1)
def shape() -> Shape:
    return Shape()


def _folds(h):
    """Deletes, sum of key_len, sum of val_len, longest key, longest value of a host record list."""
    return [int((h[:, 2] == U64_MAX).sum()), int(h[:, 1].sum(dtype=np.uint64)), int(h[:, 3].sum(dtype=np.uint64)),
            int(h[:, 1].max()), int(h[:, 3].max())]


class ThreadCase:
    """Everything thread t reads, and every word it must get."""

    def __init__(self, t: int):
        sh = shape()
        self.t = t
        rng = np.random.default_rng(1000 * (t + 1))
        self.rng = rng
        self.tag = rng.integers(97, 123, 5, dtype=np.uint8).tobytes()
        self._levels(sh)
        self._queries(sh)
        self._write_path(sh)
        self._read_path()
        self._images(sh)
        self._hashing(sh)

    def key(self, i: int) -> bytes:
        return self.tag + b"%011d" % i

    def _bytes(self, n: int) -> bytes:
        return self.rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    # --------------------------------------------------------------- level lists
    def _levels(self, sh):
        """One source, three sorted lists over it: level 0 the newest."""
        items, cuts = [], []
        for ids, dele, vlen in zip(sh.level_ids, sh.level_del, sh.level_vlen):
            pool = self._bytes(int(vlen.sum()))
            at = np.concatenate([[0], np.cumsum(vlen)])
            level = [(self.key(int(i)), None if d else pool[at[j]:at[j + 1]])
                     for j, (i, d) in enumerate(zip(ids.tolist(), dele.tolist()))]
            items += [level[j] for j in self.rng.permutation(len(level))]     # this thread's layout of the source
            cuts.append(len(items))
        case = mc.from_items("thread%d" % self.t, items, cuts=cuts[:-1])
        self.src = case.src
        self.levels = fc.split_levels(case)                # [(recs uint64 [n, 4], 0)], keys ascending
        assert [len(r) for r, _ in self.levels] == [LEVEL_N] * K
        # the merge takes the oldest list first: the newest record of a key wins
        self.merge_case = mc.Case("merge%d" % self.t, self.src, self.levels[::-1])

    def _queries(self, sh):
        keys = [self.key(int(i)) for i in sh.query_ids[self.rng.permutation(NQ)]]
        self.qsrc, self.queries = fc.lay_queries(keys)
        pre = [self.key(i)[:5 + d] for d, i in sh.prefixes]
        self.psrc, self.prefixes = fc.lay_queries([pre[j] for j in self.rng.permutation(N_PREFIX)])

    # ---------------------------------------------------------------- write path
    def _write_path(self, sh):
        self.merged, self.merge_res = self.merge_case.model(False)
        n = len(self.merged)
        assert n == sh.n_out == self.merge_res[1] and self.merge_res[3] > 100 and self.merge_res[6] > 5000
        self.pack_want = np.frombuffer(pc.packed_file(ri.as_pairs(self.src, self.merged), UUID, STARTIDX, ENDIDX),
                                       np.uint8)
        img = self.pack_want.tobytes()
        ptrs, region = zf.packed_check(img)
        assert ptrs["ok"] and region["ok"] and region["span_off"] == 40
        self.pack_res = [0, n, len(img), region["span_len"], oracle.crc32c_hw(0, img[40:40 + region["span_len"]]),
                         oracle.crc32c_hw(0, img[ptrs["span_off"]:ptrs["span_off"] + ptrs["span_len"]]),
                         region["stored"], ptrs["stored"]]
        self.pack_cap = repack.device_pack_bound(n, self.merge_res[4], self.merge_res[5])
        assert len(self.pack_want) + 64 <= self.pack_cap
        sizes = [sh.tx_sizes[j] for j in self.rng.permutation(len(sh.tx_sizes))]
        self.tx_end = np.cumsum(sizes).astype(np.uint64)
        self.n_tx = len(sizes)
        self.log_cap = zsfile.device_log_bound(n, self.n_tx, self.merge_res[4], self.merge_res[5])
        log = zsfile.log(self.src, self.merged, self.tx_end, UUID, STARTIDX, ENDIDX,
                         out=np.zeros(self.log_cap, np.uint8), spans=True)
        assert log["code"] == 0 and log["commits"] == self.n_tx and log["end"] + 64 <= self.log_cap
        self.log_want = log["image"].copy()
        self.log_spans = (log["span_off"].copy(), log["span_len"].copy())
        self.log_res = log["res"].copy()

    # ----------------------------------------------------------------- read path
    def _read_path(self):
        lv = self.levels
        self.hits, self.find_res = zsfile.find(self.src, lv, self.qsrc, self.queries)
        assert int(self.find_res[0]) == 0 and int(self.find_res[4]) == NQ // 2 and int(self.find_res[3]) > 100
        self.g_values, self.g_offs, self.g_crcs, self.g_res = zsfile.gather(self.src, self.hits, crcs=True,
                                                                            cap=GATHER_CAP)
        assert int(self.g_res[0]) == 0 and 1000 < int(self.g_res[3]) <= GATHER_CAP - 64
        rows, self.s_offs, seq, self.s_res = zsfile.scan(self.src, lv, self.psrc, self.prefixes, cap=SCAN_CAP)
        n = int(self.s_res[2])
        assert int(self.s_res[0]) == 0 and 3000 < n <= SCAN_CAP - 8 and int(self.s_res[3]) <= CAND_CAP
        assert int(self.s_res[4]) > 1000 and int(self.s_res[5]) > 100      # superseded copies, winning deletes
        self.s_rows, self.s_seq = rows[:n].copy(), seq[:n].copy()
        self.next = {p: zsfile.next_(self.src, lv, self.qsrc, self.queries, page=p) for p in PAGES}
        for p, (_, _, _, res) in self.next.items():
            # most queries fill their page; those above the last key end END
            assert int(res[0]) == 0 and int(res[2]) > NQ * p // 2 and int(res[5]) > 100 and int(res[10]) > 100, (p, res)

    # -------------------------------------------------------------------- images
    def _image(self, schedule, idx, finalise=False):
        recs, sizes = schedule
        recs = [recs[j] for j in self.rng.permutation(len(recs))]
        pool, used = self._bytes(sum(max(v, 0) for _, v in recs)), 0
        w, at = zf.FileWriter(UUID, idx=idx), 0
        for n in sizes:
            for i, vlen in recs[at:at + n]:
                if vlen < 0:
                    w.remove(self.key(i))
                else:
                    w.add(self.key(i), pool[used:used + vlen])
                    used += vlen
            w.commit()
            at += n
        if finalise:
            w.finalise()
        return w.image()

    def _images(self, sh):
        active = self._image(sh.images[0], 3)
        final = self._image(sh.images[1], 1, finalise=True)
        small = bytearray(self._image(sh.images[2], 4))
        bad = zf.walk(bytes(small))[0][BAD_COMMIT + self.t]
        small[bad["span_off"] + 24 + 7] ^= 0x04          # a byte of the span's first key: the lists stay as they are
        self.active = np.frombuffer(active, np.uint8)
        assert len(active) > 4 * WALK_BLOCK
        self.rec_want, rc = ri.host_records(active, zsfile.ACTIVE)
        assert rc == zsfile.END and len(self.rec_want) == ACTIVE_N
        self.rec_res = [rc, ACTIVE_N, len(active)] + _folds(self.rec_want) + [U64_MAX, 0, 0, 0]
        images = [active, final, bytes(small)]
        parts, self.descs, pos = [], [], 0
        for gap, img in zip(GAPS, images):
            parts += [b"\xA5" * gap, img]
            pos += gap
            self.descs.append((pos, len(img)))
            pos += len(img)
        assert all(off % 8 for off, _ in self.descs)
        self.arena = np.frombuffer(b"".join(parts) + b"\xA5" * 72, np.uint8)
        offs, lens, imgs, wrows, recs, rrows, self.reports = [], [], [], [], [], [], []
        first_w = first_r = 0
        for j, (img, (at, _)) in enumerate(zip(images, self.descs)):
            off, ln, rc, end = wi.host_walk(img)
            assert (rc, end) == (zsfile.END, len(img))
            offs.append(off + np.uint64(at))
            lens.append(ln)
            imgs.append(np.full(len(off), j, np.uint32))
            wrows.append([rc, len(off), end, int(ln.max()), int(ln.min()), U64_MAX, first_w, 0])
            first_w += len(off)
            h, rc = ri.host_records(img, zsfile.ACTIVE)
            assert rc == zsfile.END
            r = h.copy()
            r[:, 0] += np.uint64(at)
            r[r[:, 2] != U64_MAX, 2] += np.uint64(at)
            recs.append(r)
            rrows.append([rc, len(h), len(img)] + _folds(h) + [U64_MAX, first_r, 0, 0])
            first_r += len(h)
            # the format oracle's verdict on every commit
            commits, end, why = zf.walk(img)
            badc = [i for i, c in enumerate(commits) if not c["ok"]]
            assert why == "end" and zf.header_check(img)[0] and len(commits) == len(off)
            self.reports.append(dict(header_rc=0, walk_rc=zsfile.END, end_off=end, n_commits=len(commits),
                                     n_bad=len(badc), first_bad=badc[0] if badc else 0))
        assert [r["n_bad"] for r in self.reports] == [0, 1, 1]
        assert self.reports[1]["first_bad"] == self.reports[1]["n_commits"] - 1       # the stale finalise commit
        assert self.reports[2]["first_bad"] == BAD_COMMIT + self.t
        ln = np.concatenate(lens)
        self.wm_want = (np.concatenate(offs), ln, np.concatenate(imgs), np.array(wrows, np.uint64),
                        [0, first_w, int(ln.max()), int(ln.min())])
        allrecs = np.concatenate(recs)
        self.rm_want = (allrecs, np.array(rrows, np.uint64), [0, first_r] + _folds(allrecs) + [0])

    # ------------------------------------------------------------------- hashing
    def _hashing(self, sh):
        self.host = self.rng.integers(0, 256, sh.b_bytes, dtype=np.uint8)
        self.b_offs, self.b_lens = sh.b_offs, sh.b_lens
        self.b_want = oracle.batch(self.host, sh.b_offs, sh.b_lens, impl="hw", threads=8)
        self.span_want = oracle.crc32c_hw(0, self.host[SPAN_OFF:SPAN_OFF + SPAN_LEN])

    # ---------------------------------------------------------------- the checks
    def scratch_needs(self) -> dict:
        """The value of every stage's *_scratch_bytes function for this thread's calls."""
        L = lib()
        small = ctypes.byref(zsfile.WalkOpts(WALK_BLOCK, WALK_TILE))
        arr, k = zsfile._walk_images(self.descs)
        n = len(self.merged)
        needs = {
            "records": L.zscrc_device_records_scratch_bytes(len(self.active), zsfile.ACTIVE, small),
            "walk_multi": L.zscrc_device_walk_multi_scratch_bytes(arr, k, small),
            "records_multi": L.zscrc_device_records_multi_scratch_bytes(arr, k, small),
            "verify_images": L.zscrc_device_walk_multi_scratch_bytes(arr, k, None),     # its walk: default geometry
            "merge": L.zscrc_device_merge_scratch_bytes(K * LEVEL_N, None),
            "pack": L.zscrc_device_pack_scratch_bytes(n, None),
            "log": L.zscrc_device_log_scratch_bytes(n, self.n_tx, None),
            "find": L.zscrc_device_find_scratch_bytes(K, None),
            "gather": L.zscrc_device_gather_scratch_bytes(NQ, None),
            "scan": L.zscrc_device_scan_scratch_bytes(N_PREFIX, K, CAND_CAP, None),
            "span": L.zscrc_span_scratch_bytes(SPAN_LEN),
        }
        for p in PAGES:
            needs["next%d" % p] = L.zscrc_device_next_scratch_bytes(NQ, K, None)
        assert all(v > 0 for v in needs.values()), needs
        return needs

    def expected(self) -> dict:
        """operation -> the arrays it must give, for the comparison between threads."""
        out = {
            "records": [self.rec_want],
            "walk_multi": list(self.wm_want[:2]),
            "records_multi": [self.rm_want[0]],
            "verify_images": [np.array([[r[k] for k in sorted(r)] for r in self.reports], np.uint64)],
            "merge": [self.merged],
            "pack": [self.pack_want],
            "log": [self.log_want],
            "log_spans": list(self.log_spans),
            "find": [self.hits],
            "gather": [self.g_values[:int(self.g_res[3])], self.g_offs, self.g_crcs],
            "scan": [self.s_rows, self.s_offs, self.s_seq],
            "batch": [self.b_want],
            "span": [np.array([self.span_want], np.uint64)],
        }
        for p, (rows, seq, cur, _) in self.next.items():
            out["next%d" % p] = [rows, seq, cur]
        return out


# The library scratch a group's calls need: group D's hashing
# calls use the DevCtx's own buffers, none of zs::Scratch.
GROUPS = {"A": ("records", "walk_multi", "records_multi", "verify_images"), "B": ("merge", "pack", "log"),
          "C": ("find", "gather", "scan") + tuple("next%d" % p for p in PAGES), "D": ()}
# the first call of each group that takes the library scratch: thread t's first one is its group's
FIRST_CALLS = ("records", "merge", "find")


@functools.lru_cache(maxsize=1)
def thread_cases() -> list:
    """The NT cases, built once a process: treat every array as read-only."""
    return [ThreadCase(t) for t in range(NT)]
