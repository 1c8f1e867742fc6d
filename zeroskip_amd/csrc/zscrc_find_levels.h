/*
 * zscrc_find_levels.h -- what the device lookup (zscrc_find.hip), the device
 * prefix scan (zscrc_scan.hip) and the successor stage (zscrc_next.hip) share:
 * the levels of a call (descriptors as zscrc_lists.h stages them), the check of
 * every level record and the splitter tables, the levels' part of the scratch,
 * the walk over the levels that are not empty, and the host code that launches
 * the check and the tables and checks the arguments their entry points take.
 * The host functions are defined once, in zscrc_find.hip, with the two kernels
 * they launch; this header declares them and holds the inline pieces each file
 * calls.
 */
#ifndef ZSCRC_FIND_LEVELS_H
#define ZSCRC_FIND_LEVELS_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/zscrc.h"
#include "zscrc_find_order.h"
#include "zscrc_internal.h"
#include "zscrc_lists.h"
#include "zscrc_wg.h"

namespace zsfind {

using zsdev::Firsts;
using zsdev::ListD;
using zsdev::N_MAX;
using zsdev::WG;
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

/* scratch words: the two minima of the check, then the caller's counters */
enum { SC_BAD = 0, SC_ORDER = 1, SC_COUNTERS = 2, SC_WORDS = 16 };

/* What the check and the table kernel read of a call. */
struct Levels {
    const uint8_t *src;
    uint64_t src_size;
    unsigned long long *sc; /* SC_WORDS words */
    ListD *levels;          /* those that are not empty and the entry that ends them */
    uint64_t *tabs;         /* filled levels x 4 S words */
    uint32_t filled;        /* levels that are not empty */
    uint32_t n;             /* n_total */
    uint32_t S;
    uint32_t check_order;
};

__device__ inline bool is_bad(const Levels &a) { return (a.sc[SC_BAD] & a.sc[SC_ORDER]) != U64_MAX; }

/* A workgroup's copy of one level's table (4 S words) into LDS; S = 1: none. */
__device__ inline void table_to_lds(uint8_t *lds, const uint64_t *tab, uint32_t S)
{
    if (S <= 1)
        return;
    const ulonglong2 *g = reinterpret_cast<const ulonglong2 *>(tab);
    ulonglong2 *s = reinterpret_cast<ulonglong2 *>(lds);
    for (uint32_t i = threadIdx.x; i < 2 * S; i += WG)
        s[i] = g[i];
    __syncthreads();
}

/* The splitters of a call; 0 = a bad option. */
inline uint32_t splitters_of(uint32_t asked) { return (uint32_t)zsdev::pow2_opt(asked, DEF_SPLITTERS, 1, S_MAX); }

/* The head of the scratch of a call with k levels into a: the words, the
 * descriptors, a table for every level. */
inline void carve_levels(Levels &a, size_t k, zs::Carve &c)
{
    a.sc = c.take<unsigned long long>(SC_WORDS, 16);
    /* 32 bytes a level, as when a descriptor carried its level's index: a ListD
     * is 24, but the documented size of the scratch stays what callers reserve */
    a.levels = reinterpret_cast<ListD *>(c.take<uint8_t>((k + 1) * 32, 16));
    a.tabs = c.take<uint64_t>(a.S > 1 ? k * 4 * (size_t)a.S : 0, 16);
}

/* The LDS of a launch that searches one level's table, and the workgroups of
 * its persistent grid for `items` items. */
inline uint32_t table_lds(uint32_t S) { return S > 1 ? S * 32 : 64; }
inline uint32_t table_grid(uint32_t S, uint64_t items)
{
    const uint32_t lds = table_lds(S);
    const uint32_t per_cu = LDS_PER_CU / lds < WG_PER_CU ? LDS_PER_CU / lds : WG_PER_CU;
    const uint32_t resident = CUS * per_cu < GRID_MAX ? CUS * per_cu : GRID_MAX;
    const uint64_t blocks = (items + WG - 1) / WG;
    return blocks < resident ? (uint32_t)blocks : resident;
}

/* The first launches of a call: the descriptors of the levels that hold
 * records to a.levels through the pinned staging, the two minima preset, the
 * check (one thread a level record: rebased and checked against the source,
 * with check_order its key against its predecessor's; thread 0 zeroes the
 * counters), the tables (one thread a splitter of every level that is not
 * empty). */
int launch_levels(const Levels &a, zs::Scratch &sc, const zscrc_merge_list *levels, size_t k, hipStream_t s);

/* f(level, l, li, tab, first, last) for every level that is not empty: its
 * index among the caller's and among those, its table, whether it is the first
 * and the last one.  None holds a record: f once with an empty level, l = k. */
template <class F>
inline void for_filled_levels(const Levels &a, const zscrc_merge_list *levels, size_t k, F f)
{
    uint32_t li = 0;
    for (size_t l = 0; l < k; ++l) {
        if (!levels[l].n)
            continue;
        f(Level{levels[l].d_recs, levels[l].n, levels[l].base}, l, li, a.tabs + (uint64_t)li * 4 * a.S, li == 0,
          li + 1 == a.filled);
        ++li;
    }
    if (!li)
        f(Level{}, k, 0u, static_cast<const uint64_t *>(nullptr), true, true);
}
/* The argument checks of the levels, the sources and the queries that the
 * device and the host entries of the lookup and of the scan share; *n_total
 * and *filled on success. */
bool levels_args_ok(const void *src, uint64_t src_size, const zscrc_merge_list *levels, size_t k, const void *qsrc,
                    uint64_t qsrc_size, const void *queries, size_t nq, uint64_t *n_total, uint32_t *filled);
/* The check of the host forms, every record of every level in seq order: the
 * smallest offending seq of each kind into res[0], [1], [7] as the seal
 * kernels write them; false = an offence. */
bool host_check(const uint8_t *src, uint64_t src_size, const zscrc_merge_list *levels, size_t k, bool check_order,
                uint64_t *res);

} /* namespace zsfind */

#endif
