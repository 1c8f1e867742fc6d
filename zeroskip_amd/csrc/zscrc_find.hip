/*
 * zscrc_find.hip -- the read path for record lists that live in device memory:
 * zscrc_device_find looks a batch of keys up in k sorted lists (levels) over
 * one source, newest first, with no key crossing PCIe ("The
 * lookup on the device"); zscrc_zs_find is the same search for lists and keys
 * in host memory.  The search arithmetic is zscrc_find_order.h's, the order
 * zscrc_merge_order.h's, both shared with the host.
 *
 * Launches, all in stream order, no workgroup waiting for another one:
 *
 *   (the first two are launched by zscrc_find_levels.h's launch_levels:
 *   zscrc_scan.hip's calls begin with them too)
 *   find_check_kernel     one thread per level record: its level by binary
 *                         search of the staged prefix counts, the record
 *                         rebased and checked against the source, with
 *                         CHECK_ORDER its key against its predecessor's in the
 *                         same level (the smallest offending seq of each kind
 *                         by an integer min); thread 0 zeroes the counters
 *   find_table_kernel     one thread per splitter of every level that is not
 *                         empty: the sampled record's key words, length and
 *                         rebased offset into the level's table
 *   find_search_kernel    once per level that is not empty, persistent
 *                         workgroups with a grid-stride loop over the queries:
 *                         the level's table copied into LDS, each thread's
 *                         query narrowed to a bucket there and the bisection
 *                         finished against the records; the first launch
 *                         initialises the hits, the last one counts them
 *   find_seal_kernel      one lane: the result words
 *
 * Every grid comes from n_total, k and nq on the host.  An offending record
 * makes every launch after the check return at once.
 *
 * The level descriptors and their staging are zscrc_lists.h's; the scratch of
 * a call is laid out by carve() on top of zscrc_find_levels.h's carve_levels.
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "../../include/zscrc.h"
#include "zscrc_find_levels.h"
#include "zscrc_find_order.h"
#include "zscrc_internal.h"
#include "zscrc_wg.h"

/* what zscrc_find_levels.h declares, and the two kernels launch_levels
 * launches: shared with zscrc_scan.hip */
namespace zsfind {

__global__ __launch_bounds__(WG) void find_check_kernel(Levels a)
{
    const uint64_t seq = (uint64_t)blockIdx.x * WG + threadIdx.x;
    if (seq == 0)
        for (int i = SC_COUNTERS; i < SC_WORDS; ++i)
            a.sc[i] = 0;
    if (seq >= a.n)
        return;
    const ListD l = a.levels[zspack::find_rec(Firsts{a.levels}, a.filled, seq)];
    const uint64_t j = seq - l.first;
    zscrc_zs_record r = l.recs[j];
    if (!zsmerge::rebase(r, l.base, a.src_size)) {
        atomicMin(a.sc + SC_BAD, (unsigned long long)seq);
        return;
    }
    if (!a.check_order || j == 0)
        return;
    zscrc_zs_record prev = l.recs[j - 1];
    /* a predecessor outside the source is its own, smaller, offence */
    if (zsmerge::rebase(prev, l.base, a.src_size) && order_offence(a.src, prev, r))
        atomicMin(a.sc + SC_ORDER, (unsigned long long)seq);
}

__global__ __launch_bounds__(WG) void find_table_kernel(Levels a)
{
    const uint64_t t = (uint64_t)blockIdx.x * WG + threadIdx.x;
    if (t >= (uint64_t)a.filled * a.S || is_bad(a))
        return;
    const uint32_t li = (uint32_t)(t / a.S), j = (uint32_t)(t % a.S);
    const ListD l = a.levels[li];
    const zscrc_zs_record r = l.recs[splitter_pos(j, a.levels[li + 1].first - l.first, a.S)];
    table_store(a.tabs + (uint64_t)li * 4 * a.S, a.S, j, a.src, r.key_off + l.base, r.key_len);
}

int launch_levels(const Levels &a, zs::Scratch &sc, const zscrc_merge_list *levels, size_t k, hipStream_t s)
{
    if (a.n) {
        const int rc = zsdev::stage_lists(sc, levels, k, a.filled, a.levels, s);
        if (rc)
            return rc;
    }
    if (hipMemsetAsync(a.sc, 0xFF, 16, s) != hipSuccess)
        return ZSCRC_EHIP;
    hipLaunchKernelGGL(find_check_kernel, dim3(a.n ? (a.n + WG - 1) / WG : 1), dim3(WG), 0, s, a);
    if (a.n && a.S > 1)
        hipLaunchKernelGGL(find_table_kernel, dim3((uint32_t)(((uint64_t)a.filled * a.S + WG - 1) / WG)), dim3(WG), 0,
                           s, a);
    return ZSCRC_OK;
}

bool levels_args_ok(const void *src, uint64_t src_size, const zscrc_merge_list *levels, size_t k, const void *qsrc,
                    uint64_t qsrc_size, const void *queries, size_t nq, uint64_t *n_total, uint32_t *filled)
{
    return !(nq && !queries) && !(!src && src_size) && !(!qsrc && qsrc_size) && src_size <= zspack::SRC_MAX &&
           qsrc_size <= zspack::SRC_MAX && nq <= N_MAX &&
           zsdev::lists_ok(levels, k, ZSCRC_FIND_LEVELS_MAX, n_total, filled);
}

bool host_check(const uint8_t *src, uint64_t src_size, const zscrc_merge_list *levels, size_t k, bool check_order,
                uint64_t *res)
{
    uint64_t bad = U64_MAX, order = U64_MAX, seq = 0;
    for (size_t l = 0; l < k; ++l)
        for (uint64_t j = 0; j < levels[l].n; ++j, ++seq) {
            zscrc_zs_record r = levels[l].d_recs[j];
            if (!zsmerge::rebase(r, levels[l].base, src_size)) {
                if (bad == U64_MAX)
                    bad = seq;
                continue;
            }
            if (!check_order || j == 0 || order != U64_MAX)
                continue;
            zscrc_zs_record prev = levels[l].d_recs[j - 1];
            if (zsmerge::rebase(prev, levels[l].base, src_size) && order_offence(src, prev, r))
                order = seq;
        }
    return !check_verdict(bad, order, res);
}

} /* namespace zsfind */

namespace {

using namespace zsfind;
using namespace zsdev;
using zsmerge::rebase;
using zspack::U64_MAX;

/* scratch words after the check's two minima: the counters of res[2] .. res[6] */
enum { SC_VALUES = SC_COUNTERS, SC_DELETES, SC_NONE, SC_BADQ, SC_SUMV };

/* A call: the levels with their check and tables (zscrc_find_levels.h), the
 * queries and the outputs. */
struct Find : Levels {
    const uint8_t *qsrc;
    uint64_t qsrc_size;
    const zscrc_zs_record *queries;
    Hit *hits;
    uint64_t *res;
    uint32_t nq;
};

/* One search launch: the level (n = 0: none holds a record), its index among
 * the caller's, its table; whether it is the first and the last launch of the
 * call, and whether the level is the caller's last one. */
struct Pass {
    Level lv;
    uint64_t level;
    const uint64_t *tab;
    uint32_t first, last, last_level;
};

__global__ __launch_bounds__(WG) void find_search_kernel(Find a, Pass p)
{
    extern __shared__ __align__(16) uint8_t lds[];
    if (is_bad(a))
        return;
    uint64_t *s_tab = reinterpret_cast<uint64_t *>(lds);
    const uint32_t S = p.lv.n ? a.S : 1;
    table_to_lds(lds, p.tab, S);
    uint64_t values = 0, deletes = 0, none = 0, badq = 0, sumv = 0;
    const uint64_t stride = (uint64_t)gridDim.x * WG;
    for (uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x; i < a.nq; i += stride) {
        Hit h{NONE, 0, 0, 0};
        bool bad = false;
        if (p.first)
            bad = !key_ok(a.queries[i].key_off, a.queries[i].key_len, a.qsrc_size);
        else
            h = a.hits[i];
        if (bad) {
            h.level = BAD_QUERY;
            a.hits[i] = h;
        } else if (h.level == NONE) {
            const Query q = make_query(a.qsrc, a.queries[i].key_off, a.queries[i].key_len);
            bool found;
            const uint64_t at = find_in_level(a.qsrc, q, a.src, p.lv, s_tab, S, &found);
            if (found)
                h = hit_of(p.lv, p.level, at);
            else
                h.location = p.last_level ? at : 0;
            if (found || p.first || p.last_level)
                a.hits[i] = h;
        }
        if (!p.last)
            continue;
        if (h.level == BAD_QUERY) {
            ++badq;
        } else if (h.level == NONE) {
            ++none;
        } else if (h.val_off == ZSCRC_ZS_DELETED) {
            ++deletes;
        } else {
            ++values;
            sumv += h.val_len;
        }
    }
    if (!p.last)
        return;
    /* the table is done with: its first words carry the sums */
    __syncthreads();
    values = wg_sum(s_tab, values);
    deletes = wg_sum(s_tab, deletes);
    none = wg_sum(s_tab, none);
    badq = wg_sum(s_tab, badq);
    sumv = wg_sum(s_tab, sumv);
    if (threadIdx.x != 0)
        return;
    if (values)
        atomicAdd(a.sc + SC_VALUES, (unsigned long long)values);
    if (deletes)
        atomicAdd(a.sc + SC_DELETES, (unsigned long long)deletes);
    if (none)
        atomicAdd(a.sc + SC_NONE, (unsigned long long)none);
    if (badq)
        atomicAdd(a.sc + SC_BADQ, (unsigned long long)badq);
    if (sumv)
        atomicAdd(a.sc + SC_SUMV, (unsigned long long)sumv);
}

__global__ void find_seal_kernel(Find a)
{
    if (threadIdx.x != 0 || blockIdx.x != 0)
        return;
    for (int i = 0; i < ZSCRC_FIND_RES_WORDS; ++i)
        a.res[i] = 0;
    if (check_verdict(a.sc[SC_BAD], a.sc[SC_ORDER], a.res))
        return;
    a.res[1] = a.nq;
    a.res[2] = a.sc[SC_VALUES];
    a.res[3] = a.sc[SC_DELETES];
    a.res[4] = a.sc[SC_NONE];
    a.res[5] = a.sc[SC_BADQ];
    a.res[6] = a.sc[SC_SUMV];
}

uint32_t splitters_of(const zscrc_find_opts *o) { return zsfind::splitters_of(o ? o->splitters : 0); }

/* The scratch of a call with k levels, its pieces into a; the bytes. */
size_t carve(Find &a, size_t k, zs::Carve c)
{
    carve_levels(a, k, c);
    return up16(c.bytes());
}

int launch(Find &a, void *scratch, zs::Scratch &sc, const zscrc_merge_list *levels, size_t k, hipStream_t s)
{
    carve(a, k, zs::Carve(scratch));
    const int rc = launch_levels(a, sc, levels, k, s);
    if (rc)
        return rc;
    if (a.nq) {
        const uint32_t lds = table_lds(a.S), grid = table_grid(a.S, a.nq);
        for_filled_levels(a, levels, k,
                          [&](const Level &lv, size_t l, uint32_t, const uint64_t *tab, bool first, bool last) {
                              /* l = k: no level holds a record, the hits and the counts all the same */
                              const Pass ps{lv, l, tab, first, last, l + 1 >= k};
                              hipLaunchKernelGGL(find_search_kernel, dim3(grid), dim3(WG), lds, s, a, ps);
                          });
    }
    hipLaunchKernelGGL(find_seal_kernel, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError() == hipSuccess ? ZSCRC_OK : ZSCRC_EHIP;
}

/* The argument checks the device and the host entry share; *n_total and
 * *filled on success. */
bool args_ok(const void *src, uint64_t src_size, const zscrc_merge_list *levels, size_t k, const void *qsrc,
             uint64_t qsrc_size, const void *queries, size_t nq, const void *hits, const void *res, unsigned flags,
             uint64_t *n_total, uint32_t *filled)
{
    return res && !(nq && !hits) && !(flags & ~ZSCRC_FIND_CHECK_ORDER) &&
           levels_args_ok(src, src_size, levels, k, qsrc, qsrc_size, queries, nq, n_total, filled);
}

} /* namespace */

extern "C" {

size_t zscrc_device_find_scratch_bytes(size_t k, const zscrc_find_opts *opts)
{
    const uint32_t S = splitters_of(opts);
    if (!S || k > ZSCRC_FIND_LEVELS_MAX)
        return 0;
    Find a{};
    a.S = S;
    return carve(a, k, zs::Carve(nullptr));
}

int zscrc_device_find(const void *d_src, uint64_t src_size, const zscrc_merge_list *levels, size_t k,
                      const void *d_qsrc, uint64_t qsrc_size, const struct zscrc_zs_record *d_queries, size_t nq,
                      zscrc_find_hit *d_hits, uint64_t *d_res, void *scratch, const zscrc_find_opts *opts,
                      unsigned flags, void *stream)
{
    static_assert(sizeof(Hit) == sizeof(zscrc_find_hit), "zscrc_find_hit is four words");
    const uint32_t S = splitters_of(opts);
    uint64_t n = 0;
    uint32_t filled = 0;
    if (!S || (reinterpret_cast<uintptr_t>(scratch) & 15) ||
        !args_ok(d_src, src_size, levels, k, d_qsrc, qsrc_size, d_queries, nq, d_hits, d_res, flags, &n, &filled))
        return ZSCRC_EINVAL;
    Find a{};
    a.src = static_cast<const uint8_t *>(d_src);
    a.src_size = src_size;
    a.qsrc = static_cast<const uint8_t *>(d_qsrc);
    a.qsrc_size = qsrc_size;
    a.queries = d_queries;
    a.hits = reinterpret_cast<Hit *>(d_hits);
    a.res = d_res;
    a.filled = filled;
    a.n = (uint32_t)n;
    a.nq = (uint32_t)nq;
    a.S = S;
    a.check_order = flags & ZSCRC_FIND_CHECK_ORDER;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return zs::with_scratch(scratch, carve(a, k, zs::Carve(nullptr)), true, s,
                            [&](void *sp, zs::Scratch *sc) { return launch(a, sp, *sc, levels, k, s); });
}

int zscrc_zs_find(const void *src, uint64_t src_size, const zscrc_merge_list *levels, size_t k, const void *qsrc,
                  uint64_t qsrc_size, const struct zscrc_zs_record *queries, size_t nq, zscrc_find_hit *hits,
                  uint64_t res[ZSCRC_FIND_RES_WORDS], unsigned flags)
{
    uint64_t n = 0;
    uint32_t filled = 0;
    if (!args_ok(src, src_size, levels, k, qsrc, qsrc_size, queries, nq, hits, res, flags, &n, &filled))
        return ZSCRC_EINVAL;
    const uint8_t *s = static_cast<const uint8_t *>(src), *qs = static_cast<const uint8_t *>(qsrc);
    memset(res, 0, ZSCRC_FIND_RES_WORDS * 8);
    if (!host_check(s, src_size, levels, k, flags & ZSCRC_FIND_CHECK_ORDER, res))
        return ZSCRC_OK;
    res[1] = nq;
    for (size_t i = 0; i < nq; ++i) {
        Hit h{NONE, 0, 0, 0};
        if (!key_ok(queries[i].key_off, queries[i].key_len, qsrc_size)) {
            h.level = BAD_QUERY;
            ++res[5];
        } else {
            const Query q = make_query(qs, queries[i].key_off, queries[i].key_len);
            for (size_t l = 0; l < k && h.level == NONE; ++l) {
                const Level lv{levels[l].d_recs, levels[l].n, levels[l].base};
                bool found;
                const uint64_t at = find_in_level(qs, q, s, lv, nullptr, 1, &found);
                if (found)
                    h = hit_of(lv, l, at);
                else
                    h.location = l + 1 == k ? at : 0;
            }
            if (h.level == NONE) {
                ++res[4];
            } else if (h.val_off == ZSCRC_ZS_DELETED) {
                ++res[3];
            } else {
                ++res[2];
                res[6] += h.val_len;
            }
        }
        memcpy(&hits[i], &h, sizeof h);
    }
    return ZSCRC_OK;
}

} /* extern "C" */
