/*
 * zscrc_next.hip -- the successor stage over record lists that live in device
 * memory: zscrc_device_next hands out, for every key of a batch, the next
 * `page` live keys after it across k sorted lists (levels), each key once from
 * the newest level that holds it, deleted keys skipped, and a cursor from which
 * the next call goes on -- what zsdb_fetchnext does over a database's files
 * ("The successor on the device"); zscrc_zs_next is the same in
 * host memory.  The arithmetic is zscrc_next_order.h's on top of
 * zscrc_find_order.h's search and zscrc_scan_order.h's row, all shared with the
 * host; the check of the levels, their splitter tables, their part of the
 * scratch and the walk over those that are not empty are the lookup's
 * (zscrc_find_levels.h).
 *
 * Launches, all in stream order, no workgroup waiting for another one:
 *
 *   find_check_kernel, find_table_kernel      zscrc_find.hip's, by launch_levels
 *   next_bounds_kernel    once per level that is not empty, persistent
 *                         workgroups with a grid-stride loop over the queries
 *                         and the level's table in LDS: the query's cursor in
 *                         that level into the (level, query) matrix
 *   next_step_kernel      one thread a query: the merge over its cursors until
 *                         the stop rule ends it, the rows, the filler slots and
 *                         the cursor written as they come, the counts summed
 *                         over the workgroup
 *   next_seal_kernel      one lane: the result words
 *
 * Every grid comes from n_total, k, nq and page on the host.  An offending
 * record makes every launch after the check return at once.
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/zscrc.h"
#include "zscrc_find_levels.h"
#include "zscrc_internal.h"
#include "zscrc_next_order.h"
#include "zscrc_wg.h"

namespace {

using namespace zsfind;
using namespace zsnext;
using namespace zsdev;

/* scratch words after the check's two minima */
enum { SC_ROWS = SC_COUNTERS, SC_STEPS, SC_SUPER, SC_DELETES, SC_BADQ, SC_SUMK, SC_SUMV, SC_ENDS, SC_MORES };
static_assert(SC_MORES < SC_WORDS, "the counters fit the scratch words the check zeroes");

/* A call: the levels with their check and tables (zscrc_find_levels.h), the
 * queries, the outputs and the cursors. */
struct Next : Levels {
    const uint8_t *qsrc;
    uint64_t qsrc_size;
    const zscrc_zs_record *queries;
    zscrc_zs_record *out;
    uint64_t *seq;          /* may be NULL */
    zscrc_next_cursor *cur;
    uint64_t *res;
    uint32_t *cursors;      /* level-major: level l (of those not empty) of query i at l * nq + i */
    uint32_t nq;
    uint32_t page;
    uint32_t max_steps;
    uint32_t inclusive;
    uint32_t keep;
};

/* One bounds launch: the level, its table, its index among the levels that
 * are not empty. */
struct Pass {
    Level lv;
    const uint64_t *tab;
    uint32_t li;
};

__global__ __launch_bounds__(WG) void next_bounds_kernel(Next a, Pass p)
{
    extern __shared__ __align__(16) uint8_t lds[];
    if (is_bad(a))
        return;
    const uint64_t *s_tab = reinterpret_cast<const uint64_t *>(lds);
    table_to_lds(lds, p.tab, a.S);
    uint32_t *row = a.cursors + (uint64_t)p.li * a.nq;
    const uint64_t stride = (uint64_t)gridDim.x * WG;
    for (uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x; i < a.nq; i += stride) {
        const uint64_t off = a.queries[i].key_off, len = a.queries[i].key_len;
        if (!key_ok(off, len, a.qsrc_size))
            continue; /* a bad query: the step kernel reads no cursor of it */
        const Query q = make_query(a.qsrc, off, len);
        bool found;
        const uint64_t lb = find_in_level(a.qsrc, q, a.src, p.lv, s_tab, a.S, &found);
        row[i] = cursor_of(lb, found, a.inclusive);
    }
}

/* Query i's column of the cursor matrix. */
struct Column {
    uint32_t *p;
    uint64_t nq;
    __device__ uint32_t get(uint32_t l) const { return p[l * nq]; }
    __device__ void set(uint32_t l, uint32_t v) { p[l * nq] = v; }
};

/* ... and a query's cursors in host memory, one a level. */
struct HostCursors {
    uint32_t *p;
    uint32_t get(uint32_t l) const { return p[l]; }
    void set(uint32_t l, uint32_t v) { p[l] = v; }
};

__global__ __launch_bounds__(WG) void next_step_kernel(Next a)
{
    __shared__ uint64_t s[WG / 64];
    if (is_bad(a))
        return;
    const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
    Tally t{0, 0, 0, 0, 0, 0};
    uint64_t badq = 0, ends = 0, mores = 0;
    if (i < a.nq) {
        zscrc_zs_record *out = a.out + i * a.page;
        uint64_t *seq = a.seq ? a.seq + i * a.page : nullptr;
        zscrc_next_cursor c = bad_cursor();
        if (!key_ok(a.queries[i].key_off, a.queries[i].key_len, a.qsrc_size)) {
            badq = 1;
        } else {
            Column col{a.cursors + i, a.nq};
            c = run_query(
                a.src, a.filled,
                [&](uint32_t l) {
                    const ListD d = a.levels[l];
                    return Level{d.recs, a.levels[l + 1].first - d.first, d.base};
                },
                col, a.page, a.max_steps, a.keep != 0, t,
                [&](uint32_t slot, const zscrc_zs_record &r, uint32_t l, uint32_t at) {
                    out[slot] = r;
                    if (seq)
                        seq[slot] = a.levels[l].first + at;
                });
            ends = c.state == ZSCRC_NEXT_END;
            mores = c.state == ZSCRC_NEXT_MORE;
        }
        for (uint64_t slot = c.count; slot < a.page; ++slot) {
            out[slot] = filler();
            if (seq)
                seq[slot] = FILLER_SEQ;
        }
        a.cur[i] = c;
    }
    const uint64_t sums[9] = {t.rows, t.steps, t.superseded, t.deletes, badq, t.sumk, t.sumv, ends, mores};
#pragma unroll
    for (int w = 0; w < 9; ++w) {
        const uint64_t v = wg_sum(s, sums[w]);
        if (threadIdx.x == 0 && v)
            atomicAdd(a.sc + SC_ROWS + w, (unsigned long long)v);
    }
}

__global__ void next_seal_kernel(Next a)
{
    if (threadIdx.x != 0 || blockIdx.x != 0)
        return;
    for (int i = 0; i < ZSCRC_NEXT_RES_WORDS; ++i)
        a.res[i] = 0;
    if (check_verdict(a.sc[SC_BAD], a.sc[SC_ORDER], a.res))
        return;
    a.res[1] = a.nq;
    a.res[2] = a.sc[SC_ROWS];
    a.res[3] = a.sc[SC_STEPS];
    a.res[4] = a.sc[SC_SUPER];
    a.res[5] = a.sc[SC_DELETES];
    a.res[6] = a.sc[SC_BADQ];
    a.res[8] = a.sc[SC_SUMK];
    a.res[9] = a.sc[SC_SUMV];
    a.res[10] = a.sc[SC_ENDS];
    a.res[11] = a.sc[SC_MORES];
}

/* The pieces of the scratch into a, each on a 16-byte boundary; the bytes.
 * The cursor matrix is sized for k levels, filled or not. */
size_t carve(Next &a, size_t k, zs::Carve c)
{
    carve_levels(a, k, c);
    a.cursors = c.take<uint32_t>((size_t)a.nq * k, 16);
    return up16(c.bytes());
}

int launch(Next &a, void *scratch, zs::Scratch &sc, const zscrc_merge_list *levels, size_t k, hipStream_t s)
{
    carve(a, k, zs::Carve(scratch));
    const int rc = launch_levels(a, sc, levels, k, s);
    if (rc)
        return rc;
    if (a.nq) {
        if (a.n) {
            const uint32_t lds = table_lds(a.S), grid = table_grid(a.S, a.nq);
            for_filled_levels(a, levels, k,
                              [&](const Level &lv, size_t, uint32_t li, const uint64_t *tab, bool, bool) {
                                  const Pass ps{lv, tab, li};
                                  hipLaunchKernelGGL(next_bounds_kernel, dim3(grid), dim3(WG), lds, s, a, ps);
                              });
        }
        hipLaunchKernelGGL(next_step_kernel, dim3((a.nq + WG - 1) / WG), dim3(WG), 0, s, a);
    }
    hipLaunchKernelGGL(next_seal_kernel, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError() == hipSuccess ? ZSCRC_OK : ZSCRC_EHIP;
}

constexpr unsigned FLAGS = ZSCRC_NEXT_INCLUSIVE | ZSCRC_NEXT_CHECK_ORDER | ZSCRC_NEXT_KEEP_DELETES;

/* The argument checks the device and the host entry share; *n_total and
 * *filled on success. */
bool args_ok(const void *src, uint64_t src_size, const zscrc_merge_list *levels, size_t k, const void *qsrc,
             uint64_t qsrc_size, const void *queries, size_t nq, uint32_t page, const void *out, const void *cur,
             const void *res, unsigned flags, uint64_t *n_total, uint32_t *filled)
{
    return res && page && page <= PAGE_MAX && !(nq && (!out || !cur)) && !(flags & ~FLAGS) &&
           levels_args_ok(src, src_size, levels, k, qsrc, qsrc_size, queries, nq, n_total, filled) &&
           (uint64_t)nq * page <= N_MAX;
}

} /* namespace */

extern "C" {

size_t zscrc_device_next_scratch_bytes(size_t nq, size_t k, const zscrc_next_opts *opts)
{
    const uint32_t S = splitters_of(opts ? opts->splitters : 0);
    if (!S || k > ZSCRC_FIND_LEVELS_MAX || nq > N_MAX)
        return 0;
    Next a{};
    a.S = S;
    a.nq = (uint32_t)nq;
    return carve(a, k, zs::Carve(nullptr));
}

int zscrc_device_next(const void *d_src, uint64_t src_size, const zscrc_merge_list *levels, size_t k,
                      const void *d_qsrc, uint64_t qsrc_size, const struct zscrc_zs_record *d_queries, size_t nq,
                      uint32_t page, struct zscrc_zs_record *d_out, uint64_t *d_seq, zscrc_next_cursor *d_cur,
                      uint64_t *d_res, void *scratch, const zscrc_next_opts *opts, unsigned flags, void *stream)
{
    const uint32_t S = splitters_of(opts ? opts->splitters : 0);
    uint64_t n = 0;
    uint32_t filled = 0;
    if (!S || (reinterpret_cast<uintptr_t>(scratch) & 15) ||
        !args_ok(d_src, src_size, levels, k, d_qsrc, qsrc_size, d_queries, nq, page, d_out, d_cur, d_res, flags, &n,
                 &filled))
        return ZSCRC_EINVAL;
    Next a{};
    a.src = static_cast<const uint8_t *>(d_src);
    a.src_size = src_size;
    a.qsrc = static_cast<const uint8_t *>(d_qsrc);
    a.qsrc_size = qsrc_size;
    a.queries = d_queries;
    a.out = d_out;
    a.seq = d_seq;
    a.cur = d_cur;
    a.res = d_res;
    a.filled = filled;
    a.n = (uint32_t)n;
    a.nq = (uint32_t)nq;
    a.page = page;
    a.max_steps = opts ? opts->max_steps : 0;
    a.inclusive = flags & ZSCRC_NEXT_INCLUSIVE;
    a.keep = flags & ZSCRC_NEXT_KEEP_DELETES;
    a.S = S;
    a.check_order = flags & ZSCRC_NEXT_CHECK_ORDER;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return zs::with_scratch(scratch, carve(a, k, zs::Carve(nullptr)), true, s,
                            [&](void *sp, zs::Scratch *sc) { return launch(a, sp, *sc, levels, k, s); });
}

int zscrc_zs_next(const void *src, uint64_t src_size, const zscrc_merge_list *levels, size_t k, const void *qsrc,
                  uint64_t qsrc_size, const struct zscrc_zs_record *queries, size_t nq, uint32_t page,
                  struct zscrc_zs_record *out, uint64_t *seq, zscrc_next_cursor *cur,
                  uint64_t res[ZSCRC_NEXT_RES_WORDS], uint32_t max_steps, unsigned flags)
{
    uint64_t n = 0;
    uint32_t filled = 0;
    if (!args_ok(src, src_size, levels, k, qsrc, qsrc_size, queries, nq, page, out, cur, res, flags, &n, &filled))
        return ZSCRC_EINVAL;
    const uint8_t *s = static_cast<const uint8_t *>(src), *qs = static_cast<const uint8_t *>(qsrc);
    const bool keep = flags & ZSCRC_NEXT_KEEP_DELETES, inclusive = flags & ZSCRC_NEXT_INCLUSIVE;
    memset(res, 0, ZSCRC_NEXT_RES_WORDS * 8);
    if (!host_check(s, src_size, levels, k, flags & ZSCRC_NEXT_CHECK_ORDER, res))
        return ZSCRC_OK;
    res[1] = nq;
    /* every level, empty or not: an empty one never has a head */
    std::vector<Level> lv(k);
    std::vector<uint64_t> first(k);
    std::vector<uint32_t> cursors(k);
    for (size_t l = 0; l < k; ++l) {
        lv[l] = Level{levels[l].d_recs, levels[l].n, levels[l].base};
        first[l] = l ? first[l - 1] + levels[l - 1].n : 0;
    }
    Tally t{0, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < nq; ++i) {
        zscrc_zs_record *o = out + i * page;
        uint64_t *sq = seq ? seq + i * page : nullptr;
        zscrc_next_cursor c = bad_cursor();
        if (!key_ok(queries[i].key_off, queries[i].key_len, qsrc_size)) {
            ++res[6];
        } else {
            const Query q = make_query(qs, queries[i].key_off, queries[i].key_len);
            for (size_t l = 0; l < k; ++l) {
                bool found;
                const uint64_t lb = find_in_level(qs, q, s, lv[l], nullptr, 1, &found);
                cursors[l] = cursor_of(lb, found, inclusive);
            }
            HostCursors hc{cursors.data()};
            c = run_query(
                s, (uint32_t)k, [&](uint32_t l) { return lv[l]; }, hc, page, max_steps, keep, t,
                [&](uint32_t slot, const zscrc_zs_record &r, uint32_t l, uint32_t at) {
                    o[slot] = r;
                    if (sq)
                        sq[slot] = first[l] + at;
                });
            res[10] += c.state == ZSCRC_NEXT_END;
            res[11] += c.state == ZSCRC_NEXT_MORE;
        }
        for (uint64_t slot = c.count; slot < page; ++slot) {
            o[slot] = filler();
            if (sq)
                sq[slot] = FILLER_SEQ;
        }
        cur[i] = c;
    }
    res[2] = t.rows;
    res[3] = t.steps;
    res[4] = t.superseded;
    res[5] = t.deletes;
    res[8] = t.sumk;
    res[9] = t.sumv;
    return ZSCRC_OK;
}

} /* extern "C" */
