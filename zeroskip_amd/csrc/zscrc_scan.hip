/*
 * zscrc_scan.hip -- ordered iteration over record lists that live in device
 * memory: zscrc_device_scan hands out, for every prefix of a batch, the keys
 * of k sorted lists (levels) that begin with it, in key order, each key once
 * from the newest level that holds it, deleted keys skipped -- what
 * zsdb_foreach does over a database's files ("The prefix scan
 * on the device"); zscrc_zs_scan is the same scan in host memory, by a merge
 * with one cursor a level.  The arithmetic is zscrc_scan_order.h's on top of
 * zscrc_find_order.h's search and zscrc_merge_order.h's order, all shared with
 * the host; the check of the levels, their splitter tables, their part of the
 * scratch and the walk over those that are not empty are the lookup's
 * (zscrc_find_levels.h).
 *
 * Launches, all in stream order, no workgroup waiting for another one:
 *
 *   find_check_kernel, find_table_kernel      zscrc_find.hip's, by launch_levels
 *   scan_bounds_kernel    once per level that is not empty, persistent
 *                         workgroups with a grid-stride loop over the queries
 *                         and the level's table in LDS: the prefix's lower
 *                         bound and the length of its range into the (query,
 *                         level) matrix; the first launch counts bad queries
 *   counts_sum_kernel, counts_scan_kernel, counts_offsets_kernel
 *                         the matrix's lengths to their exclusive prefix: each
 *                         pair's first candidate, and C, the candidates
 *   slots_init_kernel     every slot "superseded"
 *   scan_rank_kernel      one thread a candidate, grid-stride over [0, C): its
 *                         pair by bisection over the prefix sums, its key
 *                         bisected in the query's range of every other level,
 *                         its slot = the sum of the bounds + the newer levels
 *                         that hold the key; the candidate's index, or a
 *                         marker, into that slot
 *   rows_sum_kernel, rows_scan_kernel, rows_scatter_kernel
 *                         the winners among the slots counted, scanned and
 *                         written as rows with their seqs, the sums beside
 *   scan_offs_kernel      one thread a query: the rows before its first slot
 *   scan_seal_kernel      one lane: the result words
 *
 * Every grid comes from n_total, k, nq and cand_cap on the host.  An offending
 * record makes every launch after the check return at once, and so does C >
 * cand_cap every launch after the counts' scan.
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/zscrc.h"
#include "zscrc_find_levels.h"
#include "zscrc_internal.h"
#include "zscrc_scan_order.h"
#include "zscrc_wg.h"

namespace {

using namespace zsfind;
using namespace zsscan;
using namespace zsdev;
using zspack::is_delete;
using zspack::U64_MAX;

/* scratch words after the check's two minima */
enum { SC_C = SC_COUNTERS, SC_ROWS, SC_DROPS, SC_DELROWS, SC_BADQ, SC_SUMK, SC_SUMV };

/* A call: the levels with their check and tables (zscrc_find_levels.h), the
 * prefixes, the outputs and the pieces of the scratch. */
struct Scan : Levels {
    const uint8_t *qsrc;
    uint64_t qsrc_size;
    const zscrc_zs_record *queries;
    zscrc_zs_record *out;
    uint64_t cap;
    uint64_t *offs;
    uint64_t *seq;  /* may be NULL */
    uint64_t *res;
    uint32_t *lo;   /* pairs: the lower bound of query q in level l at q * filled + l */
    uint64_t *start; /* pairs + 1: the range's length, then the first candidate */
    uint64_t *bs1;  /* a sum per BLOCK_RECS pairs */
    uint32_t *slots; /* cand_cap */
    uint64_t *bs2;  /* a sum per BLOCK_RECS slots */
    uint64_t pairs; /* nq * filled */
    uint32_t nq;
    uint32_t cand_cap;
    uint32_t keep;
};

/* One bounds launch: the level, its table, its index among the levels that
 * are not empty (n = 0: none is), whether it is the call's first. */
struct Pass {
    Level lv;
    const uint64_t *tab;
    uint32_t li, first;
};

/* after the counts' scan: nothing more to do */
__device__ inline bool is_over(const Scan &a) { return is_bad(a) || a.sc[SC_C] > a.cand_cap; }

__device__ inline Level level_of(const Scan &a, uint32_t li)
{
    const ListD l = a.levels[li];
    return Level{l.recs, a.levels[li + 1].first - l.first, l.base};
}

__global__ __launch_bounds__(WG) void scan_bounds_kernel(Scan a, Pass p)
{
    extern __shared__ __align__(16) uint8_t lds[];
    if (is_bad(a))
        return;
    uint64_t *s_tab = reinterpret_cast<uint64_t *>(lds);
    const uint32_t S = p.lv.n ? a.S : 1;
    table_to_lds(lds, p.tab, S);
    uint64_t badq = 0;
    const uint64_t stride = (uint64_t)gridDim.x * WG;
    for (uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x; i < a.nq; i += stride) {
        const uint64_t off = a.queries[i].key_off, len = a.queries[i].key_len;
        uint64_t lo = 0, hi = 0;
        if (!key_ok(off, len, a.qsrc_size)) {
            ++badq;
        } else if (p.lv.n) {
            const Query q = make_query(a.qsrc, off, len);
            bool found;
            lo = find_in_level(a.qsrc, q, a.src, p.lv, s_tab, S, &found);
            hi = prefix_end(a.qsrc, q, a.src, p.lv, s_tab, S, lo);
        }
        if (p.lv.n) {
            a.lo[i * a.filled + p.li] = (uint32_t)lo;
            a.start[i * a.filled + p.li] = hi - lo;
        }
    }
    if (!p.first)
        return;
    /* the table is done with: its first words carry the sum */
    __syncthreads();
    badq = wg_sum(s_tab, badq);
    if (threadIdx.x == 0 && badq)
        atomicAdd(a.sc + SC_BADQ, (unsigned long long)badq);
}

/* A block's BLOCK_RECS counts of the n, PER a thread: their sum ... */
template <class Load>
__device__ inline uint64_t block_sum(uint64_t *s, uint64_t n, Load load)
{
    const uint64_t first = (uint64_t)blockIdx.x * BLOCK_RECS + threadIdx.x * PER;
    uint64_t v = 0;
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k)
        v += first + k < n ? load(first + k) : 0;
    return wg_sum(s, v);
}
/* ... and each one's exclusive prefix on top of `before`, store(i, prefix). */
template <class Load, class Store>
__device__ inline void block_offsets(uint64_t *s, uint64_t n, uint64_t before, Load load, Store store)
{
    const uint64_t first = (uint64_t)blockIdx.x * BLOCK_RECS + threadIdx.x * PER;
    uint64_t v[PER], mine = 0, total;
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k) {
        v[k] = first + k < n ? load(first + k) : 0;
        mine += v[k];
    }
    uint64_t at = before + wg_scan(s, mine, total);
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k) {
        if (first + k < n)
            store(first + k, at);
        at += v[k];
    }
}

__global__ __launch_bounds__(WG) void counts_sum_kernel(Scan a)
{
    __shared__ uint64_t s[WG / 64];
    if (is_bad(a))
        return;
    const uint64_t sum = block_sum(s, a.pairs, [&](uint64_t i) { return a.start[i]; });
    if (threadIdx.x == 0)
        a.bs1[blockIdx.x] = sum;
}

__global__ __launch_bounds__(WG) void counts_scan_kernel(Scan a)
{
    __shared__ uint64_t s[WG / 64];
    if (is_bad(a))
        return;
    const uint64_t total = scan_counts(
        s, (a.pairs + BLOCK_RECS - 1) / BLOCK_RECS, [&](uint64_t i) { return a.bs1[i]; },
        [&](uint64_t i, uint64_t at) { a.bs1[i] = at; });
    if (threadIdx.x == 0) {
        a.sc[SC_C] = total;
        a.start[a.pairs] = total;
    }
}

__global__ __launch_bounds__(WG) void counts_offsets_kernel(Scan a)
{
    __shared__ uint64_t s[WG / 64];
    if (is_bad(a))
        return;
    block_offsets(
        s, a.pairs, a.bs1[blockIdx.x], [&](uint64_t i) { return a.start[i]; },
        [&](uint64_t i, uint64_t at) { a.start[i] = at; });
}

__global__ __launch_bounds__(WG) void slots_init_kernel(Scan a)
{
    if (is_over(a))
        return;
    const uint64_t C = a.sc[SC_C], stride = (uint64_t)gridDim.x * WG;
    for (uint64_t c = (uint64_t)blockIdx.x * WG + threadIdx.x; c < C; c += stride)
        a.slots[c] = SLOT_SUPERSEDED;
}

__global__ __launch_bounds__(WG) void scan_rank_kernel(Scan a)
{
    if (is_over(a))
        return;
    const uint64_t C = a.sc[SC_C], stride = (uint64_t)gridDim.x * WG;
    const uint32_t F = a.filled;
    for (uint64_t c = (uint64_t)blockIdx.x * WG + threadIdx.x; c < C; c += stride) {
        const Cand d = decompose(a.start, a.lo, a.pairs, F, c);
        const Level lv = level_of(a, d.level);
        const zscrc_zs_record rec = lv.recs[d.rec];
        const Query key = make_query(a.src, rec.key_off + lv.base, rec.key_len);
        const uint64_t row = d.query * F;
        const Rank r = rank_of(d, a.start, a.lo, F, [&](uint32_t m, uint64_t cnt, uint64_t *lb, bool *found) {
            bound_in_range(a.src, key, level_of(a, m), a.lo[row + m], cnt, lb, found);
        });
        const uint64_t first = a.start[row];
        uint64_t slot;
        /* first + count <= C <= cand_cap: the slot lies inside the slots */
        if (slot_of(r, first, a.start[row + F] - first, &slot))
            a.slots[slot] = slot_value((uint32_t)c, r.superseded, is_delete(rec), a.keep);
    }
}

__device__ inline bool is_row(uint32_t slot) { return slot < SLOT_DROPPED; }

__global__ __launch_bounds__(WG) void rows_sum_kernel(Scan a)
{
    __shared__ uint64_t s[WG / 64];
    if (is_over(a))
        return;
    const uint64_t C = a.sc[SC_C];
    if ((uint64_t)blockIdx.x * BLOCK_RECS >= C)
        return;
    uint64_t drops = 0;
    const uint64_t rows = block_sum(s, C, [&](uint64_t i) {
        const uint32_t v = a.slots[i];
        drops += v == SLOT_DROPPED;
        return (uint64_t)is_row(v);
    });
    drops = wg_sum(s, drops);
    if (threadIdx.x != 0)
        return;
    a.bs2[blockIdx.x] = rows;
    if (drops)
        atomicAdd(a.sc + SC_DROPS, (unsigned long long)drops);
}

__global__ __launch_bounds__(WG) void rows_scan_kernel(Scan a)
{
    __shared__ uint64_t s[WG / 64];
    if (is_over(a))
        return;
    const uint64_t total = scan_counts(
        s, (a.sc[SC_C] + BLOCK_RECS - 1) / BLOCK_RECS, [&](uint64_t i) { return a.bs2[i]; },
        [&](uint64_t i, uint64_t at) { a.bs2[i] = at; });
    if (threadIdx.x == 0)
        a.sc[SC_ROWS] = total;
}

__global__ __launch_bounds__(WG) void rows_scatter_kernel(Scan a)
{
    __shared__ uint64_t s[WG / 64];
    if (is_over(a))
        return;
    const uint64_t C = a.sc[SC_C];
    if ((uint64_t)blockIdx.x * BLOCK_RECS >= C)
        return;
    uint64_t sumk = 0, sumv = 0, dels = 0;
    block_offsets(
        s, C, a.bs2[blockIdx.x], [&](uint64_t i) { return (uint64_t)is_row(a.slots[i]); },
        [&](uint64_t i, uint64_t at) {
            const uint32_t c = a.slots[i];
            if (!is_row(c) || c >= C)
                return;
            const Cand d = decompose(a.start, a.lo, a.pairs, a.filled, c);
            const zscrc_zs_record r = row_of(level_of(a, d.level), d.rec);
            sumk += r.key_len;
            if (is_delete(r))
                ++dels;
            else
                sumv += r.val_len;
            if (at >= a.cap)
                return;
            a.out[at] = r;
            if (a.seq)
                a.seq[at] = a.levels[d.level].first + d.rec;
        });
    sumk = wg_sum(s, sumk);
    sumv = wg_sum(s, sumv);
    dels = wg_sum(s, dels);
    if (threadIdx.x != 0)
        return;
    if (sumk)
        atomicAdd(a.sc + SC_SUMK, (unsigned long long)sumk);
    if (sumv)
        atomicAdd(a.sc + SC_SUMV, (unsigned long long)sumv);
    if (dels)
        atomicAdd(a.sc + SC_DELROWS, (unsigned long long)dels);
}

__global__ __launch_bounds__(WG) void scan_offs_kernel(Scan a)
{
    const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
    if (i > a.nq || is_over(a))
        return;
    /* start[nq * filled] = C: the entry past the last query is the total */
    const uint64_t C = a.sc[SC_C], at = a.start[i * a.filled];
    uint64_t rows = a.sc[SC_ROWS];
    if (at < C) {
        const uint64_t b = at / BLOCK_RECS;
        rows = a.bs2[b];
        /* the block's slots before `at`: at most 255 16-byte loads (the slots
         * and a block's first one are 16-byte aligned), then at most 3 slots */
        uint64_t j = b * BLOCK_RECS;
        for (; j + 4 <= at; j += 4) {
            const uint4 v = *reinterpret_cast<const uint4 *>(a.slots + j);
            rows += is_row(v.x) + is_row(v.y) + is_row(v.z) + is_row(v.w);
        }
        for (; j < at; ++j)
            rows += is_row(a.slots[j]);
    }
    a.offs[i] = rows;
}

__global__ void scan_seal_kernel(Scan a)
{
    if (threadIdx.x != 0 || blockIdx.x != 0)
        return;
    for (int i = 0; i < ZSCRC_SCAN_RES_WORDS; ++i)
        a.res[i] = 0;
    if (check_verdict(a.sc[SC_BAD], a.sc[SC_ORDER], a.res))
        return;
    const uint64_t C = a.sc[SC_C];
    a.res[1] = a.nq;
    a.res[3] = C;
    a.res[6] = a.sc[SC_BADQ];
    if (C > a.cand_cap) {
        a.res[0] = ZSCRC_ZS_OVERFLOW;
        a.res[7] = 1;
        return;
    }
    const uint64_t rows = a.sc[SC_ROWS], drops = a.sc[SC_DROPS];
    a.res[0] = rows > a.cap ? ZSCRC_ZS_OVERFLOW : 0;
    a.res[2] = rows;
    a.res[4] = C - rows - drops;
    a.res[5] = a.keep ? a.sc[SC_DELROWS] : drops;
    a.res[8] = a.sc[SC_SUMK];
    a.res[9] = a.sc[SC_SUMV];
}

/* The pieces of the scratch into a, each on a 16-byte boundary; the bytes.
 * The (query, level) matrix is sized for k levels, filled or not. */
size_t carve(Scan &a, size_t k, zs::Carve c)
{
    const size_t pairs = (size_t)a.nq * k;
    carve_levels(a, k, c);
    a.lo = c.take<uint32_t>(pairs, 16);
    a.start = c.take<uint64_t>(pairs + 1, 16);
    a.bs1 = c.take<uint64_t>(pairs / BLOCK_RECS + 1, 16);
    a.slots = c.take<uint32_t>(a.cand_cap, 16);
    a.bs2 = c.take<uint64_t>(a.cand_cap / BLOCK_RECS + 1, 16);
    return up16(c.bytes());
}

int launch(Scan &a, void *scratch, zs::Scratch &sc, const zscrc_merge_list *levels, size_t k, hipStream_t s)
{
    carve(a, k, zs::Carve(scratch));
    const int rc = launch_levels(a, sc, levels, k, s);
    if (rc)
        return rc;
    if (a.nq) {
        const uint32_t lds = table_lds(a.S), grid = table_grid(a.S, a.nq);
        for_filled_levels(a, levels, k,
                          [&](const Level &lv, size_t, uint32_t li, const uint64_t *tab, bool first, bool) {
                              /* an empty level: none holds a record, the bad queries all the same */
                              const Pass ps{lv, tab, li, first};
                              hipLaunchKernelGGL(scan_bounds_kernel, dim3(grid), dim3(WG), lds, s, a, ps);
                          });
    }
    const uint32_t pair_blocks = (uint32_t)((a.pairs + BLOCK_RECS - 1) / BLOCK_RECS);
    if (pair_blocks)
        hipLaunchKernelGGL(counts_sum_kernel, dim3(pair_blocks), dim3(WG), 0, s, a);
    hipLaunchKernelGGL(counts_scan_kernel, dim3(1), dim3(WG), 0, s, a);
    if (pair_blocks)
        hipLaunchKernelGGL(counts_offsets_kernel, dim3(pair_blocks), dim3(WG), 0, s, a);
    if (a.cand_cap && a.pairs) {
        const uint32_t blocks = (a.cand_cap + WG - 1) / WG, grid = blocks < GRID_MAX ? blocks : GRID_MAX;
        const uint32_t slot_blocks = (a.cand_cap + BLOCK_RECS - 1) / BLOCK_RECS;
        hipLaunchKernelGGL(slots_init_kernel, dim3(grid), dim3(WG), 0, s, a);
        hipLaunchKernelGGL(scan_rank_kernel, dim3(grid), dim3(WG), 0, s, a);
        hipLaunchKernelGGL(rows_sum_kernel, dim3(slot_blocks), dim3(WG), 0, s, a);
        hipLaunchKernelGGL(rows_scan_kernel, dim3(1), dim3(WG), 0, s, a);
        hipLaunchKernelGGL(rows_scatter_kernel, dim3(slot_blocks), dim3(WG), 0, s, a);
    }
    hipLaunchKernelGGL(scan_offs_kernel, dim3(a.nq / WG + 1), dim3(WG), 0, s, a);
    hipLaunchKernelGGL(scan_seal_kernel, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError() == hipSuccess ? ZSCRC_OK : ZSCRC_EHIP;
}

constexpr unsigned FLAGS = ZSCRC_SCAN_KEEP_DELETES | ZSCRC_SCAN_CHECK_ORDER;

/* The argument checks the device and the host entry share; *n_total and
 * *filled on success. */
bool args_ok(const void *src, uint64_t src_size, const zscrc_merge_list *levels, size_t k, const void *qsrc,
             uint64_t qsrc_size, const void *queries, size_t nq, const void *out, size_t cap, const void *offs,
             const void *res, unsigned flags, uint64_t *n_total, uint32_t *filled)
{
    return res && offs && !(cap && !out) && !(flags & ~FLAGS) &&
           levels_args_ok(src, src_size, levels, k, qsrc, qsrc_size, queries, nq, n_total, filled);
}

} /* namespace */

extern "C" {

size_t zscrc_device_scan_scratch_bytes(size_t nq, size_t k, size_t cand_cap, const zscrc_scan_opts *opts)
{
    const uint32_t S = splitters_of(opts ? opts->splitters : 0);
    if (!S || k > ZSCRC_FIND_LEVELS_MAX || nq > N_MAX || cand_cap > N_MAX)
        return 0;
    Scan a{};
    a.S = S;
    a.nq = (uint32_t)nq;
    a.cand_cap = (uint32_t)cand_cap;
    return carve(a, k, zs::Carve(nullptr));
}

int zscrc_device_scan(const void *d_src, uint64_t src_size, const zscrc_merge_list *levels, size_t k,
                      const void *d_qsrc, uint64_t qsrc_size, const struct zscrc_zs_record *d_queries, size_t nq,
                      struct zscrc_zs_record *d_out, size_t cap, uint64_t *d_offs, uint64_t *d_seq, uint64_t *d_res,
                      void *scratch, size_t cand_cap, const zscrc_scan_opts *opts, unsigned flags, void *stream)
{
    const uint32_t S = splitters_of(opts ? opts->splitters : 0);
    uint64_t n = 0;
    uint32_t filled = 0;
    if (!S || (reinterpret_cast<uintptr_t>(scratch) & 15) || cand_cap > N_MAX ||
        !args_ok(d_src, src_size, levels, k, d_qsrc, qsrc_size, d_queries, nq, d_out, cap, d_offs, d_res, flags, &n,
                 &filled))
        return ZSCRC_EINVAL;
    Scan a{};
    a.src = static_cast<const uint8_t *>(d_src);
    a.src_size = src_size;
    a.qsrc = static_cast<const uint8_t *>(d_qsrc);
    a.qsrc_size = qsrc_size;
    a.queries = d_queries;
    a.out = d_out;
    a.cap = cap;
    a.offs = d_offs;
    a.seq = d_seq;
    a.res = d_res;
    a.filled = filled;
    a.n = (uint32_t)n;
    a.nq = (uint32_t)nq;
    a.pairs = (uint64_t)nq * filled;
    a.cand_cap = (uint32_t)cand_cap;
    a.keep = flags & ZSCRC_SCAN_KEEP_DELETES;
    a.S = S;
    a.check_order = flags & ZSCRC_SCAN_CHECK_ORDER;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return zs::with_scratch(scratch, carve(a, k, zs::Carve(nullptr)), true, s,
                            [&](void *sp, zs::Scratch *sc) { return launch(a, sp, *sc, levels, k, s); });
}

int zscrc_zs_scan(const void *src, uint64_t src_size, const zscrc_merge_list *levels, size_t k, const void *qsrc,
                  uint64_t qsrc_size, const struct zscrc_zs_record *queries, size_t nq, struct zscrc_zs_record *out,
                  size_t cap, uint64_t *offs, uint64_t *seq, uint64_t res[ZSCRC_SCAN_RES_WORDS], unsigned flags)
{
    uint64_t n = 0;
    uint32_t filled = 0;
    if (!args_ok(src, src_size, levels, k, qsrc, qsrc_size, queries, nq, out, cap, offs, res, flags, &n, &filled))
        return ZSCRC_EINVAL;
    const uint8_t *s = static_cast<const uint8_t *>(src), *qs = static_cast<const uint8_t *>(qsrc);
    const bool keep = flags & ZSCRC_SCAN_KEEP_DELETES;
    memset(res, 0, ZSCRC_SCAN_RES_WORDS * 8);
    if (!host_check(s, src_size, levels, k, flags & ZSCRC_SCAN_CHECK_ORDER, res))
        return ZSCRC_OK;
    res[1] = nq;
    std::vector<Level> lv(k);
    std::vector<uint64_t> first(k), cur(k), end(k);
    for (size_t l = 0; l < k; ++l) {
        lv[l] = Level{levels[l].d_recs, levels[l].n, levels[l].base};
        first[l] = l ? first[l - 1] + levels[l - 1].n : 0;
    }
    const auto key_of = [&](size_t l) {
        const zscrc_zs_record &r = lv[l].recs[cur[l]];
        return make_query(s, r.key_off + lv[l].base, r.key_len);
    };
    uint64_t rows = 0;
    for (size_t i = 0; i < nq; ++i) {
        offs[i] = rows;
        if (!key_ok(queries[i].key_off, queries[i].key_len, qsrc_size)) {
            ++res[6];
            continue;
        }
        const Query p = make_query(qs, queries[i].key_off, queries[i].key_len);
        for (size_t l = 0; l < k; ++l) {
            bool found;
            cur[l] = find_in_level(qs, p, s, lv[l], nullptr, 1, &found);
            end[l] = prefix_end(qs, p, s, lv[l], nullptr, 1, cur[l]);
            res[3] += end[l] - cur[l];
        }
        /* the merge: one cursor a level, the smallest key from the first level that holds it */
        for (;;) {
            size_t best = k;
            Query key{};
            for (size_t l = 0; l < k; ++l) {
                if (cur[l] == end[l])
                    continue;
                const zscrc_zs_record &r = lv[l].recs[cur[l]];
                if (best == k || cmp_key(s, key, s, r.key_off + lv[l].base, r.key_len) > 0) {
                    best = l;
                    key = key_of(l);
                }
            }
            if (best == k)
                break;
            for (size_t l = best + 1; l < k; ++l) {
                if (cur[l] == end[l])
                    continue;
                const zscrc_zs_record &r = lv[l].recs[cur[l]];
                if (cmp_key(s, key, s, r.key_off + lv[l].base, r.key_len) == 0) {
                    ++cur[l];
                    ++res[4];
                }
            }
            const uint64_t at = cur[best]++;
            const zscrc_zs_record r = row_of(lv[best], at);
            const bool del = is_delete(r);
            res[5] += del;
            if (del && !keep)
                continue;
            if (rows < cap) {
                out[rows] = r;
                if (seq)
                    seq[rows] = first[best] + at;
            }
            ++rows;
            res[8] += r.key_len;
            if (!del)
                res[9] += r.val_len;
        }
    }
    offs[nq] = rows;
    res[2] = rows;
    if (rows > cap)
        res[0] = ZSCRC_ZS_OVERFLOW;
    return ZSCRC_OK;
}

} /* extern "C" */
