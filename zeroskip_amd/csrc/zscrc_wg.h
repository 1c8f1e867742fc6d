/*
 * zscrc_wg.h -- the workgroup primitives of the device stages (zscrc_walk.hip,
 * zscrc_devpack.hip, zscrc_merge.hip, zscrc_find.hip, zscrc_gather.hip,
 * zscrc_scan.hip, zscrc_next.hip, zscrc_devlog.hip): a sum, an exclusive prefix sum and the one-workgroup scan of
 * a long array of counts, and the 16-byte word of the tiled copies.  Device
 * code only, for workgroups of WG = 256 threads in waves of 64.
 *
 * Every function takes s, WG / 64 words of LDS that are free again on return,
 * is called by all threads of the workgroup, and takes the addition as a
 * functor: plain + (Plus) or one that saturates (SatAdd, for sums of lengths).
 * An addition must be associative and commutative with 0 as its identity.
 */
#ifndef ZSCRC_WG_H
#define ZSCRC_WG_H

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "zscrc_internal.h"
#include "zscrc_pack_layout.h"

namespace zsdev {

/* two words stored as one aligned 16-byte word (pack_copy_kernel, log_copy_kernel, gather's store_word) */
typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

constexpr uint32_t SCAN_PER = 4; /* scan_counts: counts a thread and chunk */

struct Plus {
    __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return a + b; }
};
/* Sums of lengths saturate (zscrc_pack_layout.h, zscrc_gather_layout.h's sum_len). */
struct SatAdd {
    __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return zspack::sat_add(a, b); }
};

/* Sum of one value a thread over the workgroup, in every thread. */
template <class Add = Plus>
__device__ inline uint64_t wg_sum(uint64_t *s, uint64_t v, Add add = Add{})
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
        v = add(v, __shfl_xor(v, d, 64));
    if ((threadIdx.x & 63) == 0)
        s[threadIdx.x >> 6] = v;
    __syncthreads();
    uint64_t all = 0;
#pragma unroll
    for (unsigned w = 0; w < WG / 64; ++w)
        all = add(all, s[w]);
    __syncthreads();
    return all;
}

/* Exclusive prefix sum of one value a thread over the workgroup; total = the
 * sum of all.  A wave's inclusive sums by shuffles, shifted by one lane (so a
 * saturated sum needs no subtraction), on top of the sums of the waves before. */
template <class Add = Plus>
__device__ inline uint64_t wg_scan(uint64_t *s, uint64_t mine, uint64_t &total, Add add = Add{})
{
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t inc = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = __shfl_up(inc, d, 64);
        if (lane >= (unsigned)d)
            inc = add(inc, o);
    }
    if (lane == 63)
        s[wave] = inc;
    const uint64_t prev = __shfl_up(inc, 1, 64);
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (unsigned w = 0; w < WG / 64; ++w) {
        if (w < wave)
            before = add(before, s[w]);
        all = add(all, s[w]);
    }
    __syncthreads();
    total = all;
    return lane ? add(before, prev) : before;
}

/* One workgroup: the n counts load(i) to their exclusive prefix, store(i,
 * prefix), in chunks of WG * SCAN_PER counts with a carry between them;
 * returns the sum of all. */
template <class Load, class Store, class Add = Plus>
__device__ inline uint64_t scan_counts(uint64_t *s, uint64_t n, Load load, Store store, Add add = Add{})
{
    uint64_t carry = 0;
    for (uint64_t c = 0; c < n; c += WG * SCAN_PER) {
        const uint64_t first = c + (uint64_t)threadIdx.x * SCAN_PER;
        uint64_t v[SCAN_PER], mine = 0;
#pragma unroll
        for (uint32_t k = 0; k < SCAN_PER; ++k) {
            v[k] = first + k < n ? load(first + k) : 0;
            mine = add(mine, v[k]);
        }
        uint64_t total;
        uint64_t at = add(carry, wg_scan(s, mine, total, add));
#pragma unroll
        for (uint32_t k = 0; k < SCAN_PER; ++k) {
            if (first + k < n)
                store(first + k, at);
            at = add(at, v[k]);
        }
        carry = add(carry, total);
    }
    return carry;
}

} /* namespace zsdev */

#endif
