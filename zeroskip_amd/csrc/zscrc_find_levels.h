/*
 * zscrc_find_levels.h -- what the device lookup (zscrc_find.hip) and the
 * device prefix scan (zscrc_scan.hip) share of their first two launches: the
 * levels as they lie on the device, the check of every level record and the
 * splitter tables, with the host code that stages the descriptors and checks
 * the arguments both entry points take.  The two kernels and the host
 * functions are defined once, in zscrc_find.hip; this header declares them and
 * holds the inline pieces a kernel of either file calls.
 */
#ifndef ZSCRC_FIND_LEVELS_H
#define ZSCRC_FIND_LEVELS_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/zscrc.h"
#include "zscrc_find_order.h"
#include "zscrc_internal.h"
#include "zscrc_wg.h"

namespace zsfind {

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

/* scratch words: the two minima of the check, then the caller's counters */
enum { SC_BAD = 0, SC_ORDER = 1, SC_COUNTERS = 2, SC_WORDS = 16 };

/* What the check and the table kernel read of a call. */
struct Levels {
    const uint8_t *src;
    uint64_t src_size;
    unsigned long long *sc; /* SC_WORDS words */
    const LevelD *levels;
    uint64_t *tabs;         /* filled levels x 4 S words */
    uint32_t filled;        /* levels that are not empty */
    uint32_t n;             /* n_total */
    uint32_t S;
    uint32_t check_order;
};

__device__ inline bool is_bad(const Levels &a) { return (a.sc[SC_BAD] & a.sc[SC_ORDER]) != U64_MAX; }

/* one thread a level record: rebased and checked against the source, with
 * check_order its key against its predecessor's; thread 0 zeroes the counters */
__global__ void find_check_kernel(Levels a);
/* one thread a splitter of every level that is not empty */
__global__ void find_table_kernel(Levels a);

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
inline uint32_t splitters_of(uint32_t asked)
{
    const uint32_t s = asked ? asked : DEF_SPLITTERS;
    return zsdev::pow2(s) && s <= S_MAX ? s : 0;
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
 * records to d_levels through the pinned staging, the two minima preset, the
 * check, the tables. */
int launch_levels(const Levels &a, LevelD *d_levels, zs::Scratch &sc, const zscrc_merge_list *levels, size_t k,
                  hipStream_t s);
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
