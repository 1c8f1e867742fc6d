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
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "../../include/zscrc.h"
#include "zscrc_find_order.h"
#include "zscrc_internal.h"
#include "zscrc_wg.h"

namespace {

using namespace zsfind;
using namespace zsdev;
using zsmerge::rebase;
using zspack::U64_MAX;

/* the default: measured, DESIGN.md 2.6 (faster than no table on random, sorted
 * and whole-list batches; 2,048 is faster still on random keys only) */
constexpr uint32_t DEF_SPLITTERS = 1024;
/* the search's persistent grid: at most this many workgroups of WG threads
 * (zsfile.FIND_GRID_THREADS mirrors the product) */
constexpr uint32_t GRID_MAX = 1024;
/* ... and no more than are resident at once with their tables: an MI355X has
 * 256 CUs of 160 KiB LDS, each holding 8 workgroups of WG threads */
constexpr uint32_t CUS = 256, LDS_PER_CU = 160 * 1024, WG_PER_CU = 8;

/* A level on the device: its records, the seq of its first one, its base,
 * its index among the caller's levels.  The entry one past the last level
 * that is not empty holds n_total. */
struct LevelD {
    const zscrc_zs_record *recs;
    uint64_t first;
    uint64_t base;
    uint64_t level;
};
struct Firsts {
    const LevelD *d;
    __host__ __device__ uint64_t operator[](uint64_t i) const { return d[i].first; }
};

/* scratch words: the two minima, then the counters of res[2] .. res[6] */
enum { SC_BAD = 0, SC_ORDER = 1, SC_VALUES = 2, SC_DELETES = 3, SC_NONE = 4, SC_BADQ = 5, SC_SUMV = 6, SC_WORDS = 16 };

struct Find {
    const uint8_t *src;
    uint64_t src_size;
    const uint8_t *qsrc;
    uint64_t qsrc_size;
    const zscrc_zs_record *queries;
    Hit *hits;
    uint64_t *res;
    unsigned long long *sc; /* SC_WORDS words */
    const LevelD *levels;
    uint64_t *tabs;         /* filled levels x 4 S words */
    uint32_t filled;        /* levels that are not empty */
    uint32_t n;             /* n_total */
    uint32_t nq;
    uint32_t S;
    uint32_t check_order;
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

__device__ inline bool is_bad(const Find &a) { return (a.sc[SC_BAD] & a.sc[SC_ORDER]) != U64_MAX; }

__global__ __launch_bounds__(WG) void find_check_kernel(Find a)
{
    const uint64_t seq = (uint64_t)blockIdx.x * WG + threadIdx.x;
    if (seq == 0)
        for (int i = SC_VALUES; i < SC_WORDS; ++i)
            a.sc[i] = 0;
    if (seq >= a.n)
        return;
    const LevelD l = a.levels[zspack::find_rec(Firsts{a.levels}, a.filled, seq)];
    const uint64_t j = seq - l.first;
    zscrc_zs_record r = l.recs[j];
    if (!rebase(r, l.base, a.src_size)) {
        atomicMin(a.sc + SC_BAD, (unsigned long long)seq);
        return;
    }
    if (!a.check_order || j == 0)
        return;
    zscrc_zs_record prev = l.recs[j - 1];
    /* a predecessor outside the source is its own, smaller, offence */
    if (rebase(prev, l.base, a.src_size) && order_offence(a.src, prev, r))
        atomicMin(a.sc + SC_ORDER, (unsigned long long)seq);
}

__global__ __launch_bounds__(WG) void find_table_kernel(Find a)
{
    const uint64_t t = (uint64_t)blockIdx.x * WG + threadIdx.x;
    if (t >= (uint64_t)a.filled * a.S || is_bad(a))
        return;
    const uint32_t li = (uint32_t)(t / a.S), j = (uint32_t)(t % a.S);
    const LevelD l = a.levels[li];
    const zscrc_zs_record r = l.recs[splitter_pos(j, a.levels[li + 1].first - l.first, a.S)];
    table_store(a.tabs + (uint64_t)li * 4 * a.S, a.S, j, a.src, r.key_off + l.base, r.key_len);
}

__global__ __launch_bounds__(WG) void find_search_kernel(Find a, Pass p)
{
    extern __shared__ __align__(16) uint8_t lds[];
    if (is_bad(a))
        return;
    uint64_t *s_tab = reinterpret_cast<uint64_t *>(lds);
    const uint32_t S = p.lv.n ? a.S : 1;
    if (S > 1) {
        const ulonglong2 *g = reinterpret_cast<const ulonglong2 *>(p.tab);
        ulonglong2 *s = reinterpret_cast<ulonglong2 *>(lds);
        for (uint32_t i = threadIdx.x; i < 2 * S; i += WG)
            s[i] = g[i];
        __syncthreads();
    }
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
    const uint64_t bad = a.sc[SC_BAD], order = a.sc[SC_ORDER];
    for (int i = 0; i < ZSCRC_FIND_RES_WORDS; ++i)
        a.res[i] = 0;
    if (bad != U64_MAX || order != U64_MAX) {
        a.res[0] = (uint64_t)(int64_t)ZSCRC_EINVAL;
        a.res[1] = bad != U64_MAX ? bad : order;
        a.res[7] = bad == U64_MAX;
        return;
    }
    a.res[1] = a.nq;
    a.res[2] = a.sc[SC_VALUES];
    a.res[3] = a.sc[SC_DELETES];
    a.res[4] = a.sc[SC_NONE];
    a.res[5] = a.sc[SC_BADQ];
    a.res[6] = a.sc[SC_SUMV];
}

/* The splitters of a call; 0 = a bad option. */
uint32_t splitters_of(const zscrc_find_opts *o)
{
    const uint32_t s = o && o->splitters ? o->splitters : DEF_SPLITTERS;
    return pow2(s) && s <= S_MAX ? s : 0;
}

/* The pieces of the scratch for k levels: the words, the descriptors of the
 * levels and the entry that ends them, a table for every level. */
struct Plan {
    size_t levels_at, tabs_at, bytes;
};
Plan plan_of(size_t k, uint32_t S)
{
    Plan p;
    p.levels_at = SC_WORDS * 8;
    p.tabs_at = p.levels_at + up16((k + 1) * sizeof(LevelD));
    p.bytes = p.tabs_at + (S > 1 ? k * 4 * (size_t)S * 8 : 0);
    return p;
}

int launch(Find &a, const Plan &p, void *scratch, zs::Scratch &sc, const zscrc_merge_list *levels, size_t k,
           hipStream_t s)
{
    uint8_t *base = static_cast<uint8_t *>(scratch);
    a.sc = reinterpret_cast<unsigned long long *>(base);
    LevelD *d_levels = reinterpret_cast<LevelD *>(base + p.levels_at);
    a.levels = d_levels;
    a.tabs = reinterpret_cast<uint64_t *>(base + p.tabs_at);
    if (a.n) {
        /* the descriptors of the levels that hold records, through the pinned staging */
        const size_t bytes = ((size_t)a.filled + 1) * sizeof(LevelD);
        int rc = zs::stage_begin(sc, bytes);
        if (rc)
            return rc;
        LevelD *h = static_cast<LevelD *>(sc.pin);
        uint64_t first = 0;
        for (size_t l = 0; l < k; ++l) {
            if (!levels[l].n)
                continue;
            *h++ = LevelD{levels[l].d_recs, first, levels[l].base, l};
            first += levels[l].n;
        }
        *h = LevelD{nullptr, first, 0, k};
        rc = zs::stage_copy(sc, d_levels, bytes, s);
        if (rc)
            return rc;
    }
    if (hipMemsetAsync(a.sc, 0xFF, 16, s) != hipSuccess)
        return ZSCRC_EHIP;
    hipLaunchKernelGGL(find_check_kernel, dim3(a.n ? (a.n + WG - 1) / WG : 1), dim3(WG), 0, s, a);
    if (a.n && a.S > 1)
        hipLaunchKernelGGL(find_table_kernel, dim3((uint32_t)(((uint64_t)a.filled * a.S + WG - 1) / WG)), dim3(WG), 0,
                           s, a);
    if (a.nq) {
        const uint32_t lds = a.S > 1 ? a.S * 32 : 64;
        const uint32_t per_cu = LDS_PER_CU / lds < WG_PER_CU ? LDS_PER_CU / lds : WG_PER_CU;
        const uint32_t resident = CUS * per_cu < GRID_MAX ? CUS * per_cu : GRID_MAX;
        const uint32_t blocks = (a.nq + WG - 1) / WG, grid = blocks < resident ? blocks : resident;
        Pass ps{};
        ps.first = 1;
        uint32_t li = 0;
        for (size_t l = 0; l < k; ++l) {
            if (!levels[l].n)
                continue;
            ps.lv = Level{levels[l].d_recs, levels[l].n, levels[l].base};
            ps.level = l;
            ps.tab = a.tabs + (uint64_t)li * 4 * a.S;
            ps.last = ++li == a.filled;
            ps.last_level = l + 1 == k;
            hipLaunchKernelGGL(find_search_kernel, dim3(grid), dim3(WG), lds, s, a, ps);
            ps.first = 0;
        }
        if (!a.filled) { /* no level holds a record: the hits and the counts all the same */
            ps.last = ps.last_level = 1;
            hipLaunchKernelGGL(find_search_kernel, dim3(grid), dim3(WG), lds, s, a, ps);
        }
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
    if (!res || (nq && (!queries || !hits)) || (k && !levels) || k > ZSCRC_FIND_LEVELS_MAX || (!src && src_size) ||
        (!qsrc && qsrc_size) || src_size > zspack::SRC_MAX || qsrc_size > zspack::SRC_MAX || nq > N_MAX ||
        (flags & ~ZSCRC_FIND_CHECK_ORDER))
        return false;
    uint64_t n = 0;
    *filled = 0;
    for (size_t l = 0; l < k; ++l) {
        if ((levels[l].n && !levels[l].d_recs) || levels[l].n > N_MAX - n)
            return false;
        n += levels[l].n;
        *filled += levels[l].n != 0;
    }
    *n_total = n;
    return true;
}

} /* namespace */

extern "C" {

size_t zscrc_device_find_scratch_bytes(size_t k, const zscrc_find_opts *opts)
{
    const uint32_t S = splitters_of(opts);
    return S && k <= ZSCRC_FIND_LEVELS_MAX ? plan_of(k, S).bytes : 0;
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
    const Plan p = plan_of(k, S);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return zs::with_scratch(scratch, p.bytes, true, s,
                            [&](void *sp, zs::Scratch *sc) { return launch(a, p, sp, *sc, levels, k, s); });
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
    /* the check: every record of every level */
    uint64_t bad = U64_MAX, order = U64_MAX, seq = 0;
    for (size_t l = 0; l < k; ++l)
        for (uint64_t j = 0; j < levels[l].n; ++j, ++seq) {
            zscrc_zs_record r = levels[l].d_recs[j];
            if (!rebase(r, levels[l].base, src_size)) {
                if (bad == U64_MAX)
                    bad = seq;
                continue;
            }
            if (!(flags & ZSCRC_FIND_CHECK_ORDER) || j == 0 || order != U64_MAX)
                continue;
            zscrc_zs_record prev = levels[l].d_recs[j - 1];
            if (rebase(prev, levels[l].base, src_size) && order_offence(s, prev, r))
                order = seq;
        }
    if (bad != U64_MAX || order != U64_MAX) {
        res[0] = (uint64_t)(int64_t)ZSCRC_EINVAL;
        res[1] = bad != U64_MAX ? bad : order;
        res[7] = bad == U64_MAX;
        return ZSCRC_OK;
    }
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
