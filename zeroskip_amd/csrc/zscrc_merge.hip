/*
 * zscrc_merge.hip -- the key merge of zscrc_zs_repack on the device:
 * zscrc_device_merge sorts device-resident record lists by key and keeps the
 * winner of every key, with no key crossing PCIe ("The merge on
 * the device").  The order arithmetic is zscrc_merge_order.h's, shared with
 * the host.
 *
 * A comparison merge sort over 16-byte sort entries {key prefix, seq, length}.
 * Launches, all in stream order, no workgroup waiting for another one:
 *
 *   merge_gather_kernel   one thread per input record: its list by binary
 *                         search of the staged prefix counts, the record
 *                         rebased and checked against the source (the smallest
 *                         bad seq by an integer min), the sort entry
 *   merge_sort_kernel     one workgroup per tile: the tile's entries and each
 *                         key's second word in LDS, a bitonic network
 *   merge_pass_kernel     ceil(log2(tiles)) times, ping-pong between two entry
 *                         arrays: a workgroup produces one tile of output from
 *                         two adjacent sorted runs -- two merge-path searches
 *                         cut its pieces of both, they are staged in LDS, every
 *                         thread finds its own cut there and merges a few
 *                         entries; a last run without a partner is copied
 *   merge_flag_kernel     one workgroup per BLOCK_RECS entries: winner,
 *                         superseded or dropped delete; the block's winners,
 *                         the totals of the result words by integer adds
 *   merge_scan_kernel     one workgroup: the block counts to their exclusive
 *                         prefix, the result words
 *   merge_scatter_kernel  one workgroup per block: the winners' rebased
 *                         records to their places in the output
 *
 * Every grid and the number of passes come from n_total on the host.  A bad
 * record makes every launch after the gather return at once.
 *
 * The sums and prefix sums are zscrc_wg.h's (merge_scan_kernel: scan_counts);
 * the list descriptors, their check and their staging are zscrc_lists.h's; the
 * scratch of a call comes through zs::with_scratch (zscrc_internal.h,
 * zscrc_scratch.cpp), laid out by carve().
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "../../include/zscrc.h"
#include "zscrc_internal.h"
#include "zscrc_lists.h"
#include "zscrc_merge_order.h"
#include "zscrc_wg.h"

namespace {

using namespace zsmerge;
using namespace zsdev;
using zspack::U64_MAX;

/* the default: measured, DESIGN.md 2.6 (sorted input is 5 % slower than at
 * 1,024, shuffled input 21 % faster) */
constexpr uint32_t DEF_TILE = 2048, TILE_MIN = 64, TILE_MAX = 2048;

/* scratch words */
enum { SC_BAD = 0, SC_DELETES = 1, SC_SUMK = 2, SC_SUMV = 3, SC_DROPPED = 4, SC_WORDS = 16 };

struct Merge {
    const uint8_t *src;
    uint64_t src_size;
    ListD *lists;      /* those that are not empty and the entry that ends them */
    uint32_t k;        /* lists that are not empty */
    uint32_t n;        /* n_total */
    uint32_t tile;
    uint32_t drop;
    uint32_t nblocks;
    unsigned long long *sc; /* SC_WORDS words */
    zscrc_zs_record *rb;    /* the rebased records by seq */
    Entry *e0, *e1;
    uint32_t *bcount;       /* nblocks + 1 */
    uint8_t *flags;         /* n */
    const Entry *sorted;    /* e0 or e1: where the last pass left the entries */
    zscrc_zs_record *out;
    uint64_t cap;
    uint64_t *res;
};

struct KeyLess {
    Keys K;
    __device__ bool operator()(const Entry &a, const Entry &b) const { return less(K, a, b); }
};

__device__ inline bool is_bad(const Merge &a) { return a.sc[SC_BAD] != U64_MAX; }

__global__ __launch_bounds__(WG) void merge_gather_kernel(Merge a)
{
    const uint64_t seq = (uint64_t)blockIdx.x * WG + threadIdx.x;
    if (seq >= a.n)
        return;
    const ListD l = a.lists[zspack::find_rec(Firsts{a.lists}, a.k, seq)];
    zscrc_zs_record r = l.recs[seq - l.first];
    if (!rebase(r, l.base, a.src_size)) {
        atomicMin(a.sc + SC_BAD, (unsigned long long)seq);
        return;
    }
    a.rb[seq] = r;
    a.e0[seq] = make_entry(a.src, r, (uint32_t)seq);
}

__global__ __launch_bounds__(WG) void merge_sort_kernel(Merge a)
{
    extern __shared__ __align__(16) uint8_t lds[];
    if (is_bad(a))
        return;
    const uint32_t T = a.tile;
    Entry *s_e = reinterpret_cast<Entry *>(lds);
    uint64_t *s_w = reinterpret_cast<uint64_t *>(s_e + T);
    const Keys K{a.src, a.rb};
    const uint64_t first = (uint64_t)blockIdx.x * T;
    for (uint32_t i = threadIdx.x; i < T; i += WG) {
        Entry e{0, SEQ_PAD, 0};
        uint64_t w = 0;
        if (first + i < a.n) {
            e = a.e0[first + i];
            if (e.len > 8)
                w = key_word(K.src, K.recs[e.seq].key_off, K.recs[e.seq].key_len, 8);
        }
        s_e[i] = e;
        s_w[i] = w;
    }
    __syncthreads();
    for (uint32_t k = 2; k <= T; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < T / 2; t += WG) {
                uint32_t lo;
                bool up;
                bitonic_pair(t, k, j, &lo, &up);
                const Entry x = s_e[lo], y = s_e[lo + j];
                const uint64_t wx = s_w[lo], wy = s_w[lo + j];
                if (less_tile(K, y, wy, x, wx) == up) {
                    s_e[lo] = y;
                    s_e[lo + j] = x;
                    s_w[lo] = wy;
                    s_w[lo + j] = wx;
                }
            }
            __syncthreads();
        }
    }
    for (uint32_t i = threadIdx.x; i < T; i += WG)
        if (first + i < a.n)
            a.e0[first + i] = s_e[i];
}

/* One pass: runs of `run` entries of `in` merged pairwise into `out`. */
__global__ __launch_bounds__(WG) void merge_pass_kernel(Merge a, const Entry *in, Entry *out, uint32_t run)
{
    extern __shared__ __align__(16) uint8_t lds[];
    __shared__ uint32_t s_cut[2];
    if (is_bad(a))
        return;
    Entry *s = reinterpret_cast<Entry *>(lds);
    const uint32_t T = a.tile, n = a.n;
    const uint64_t o0 = (uint64_t)blockIdx.x * T;          /* the output tile [o0, o0 + cnt) */
    const uint32_t cnt = n - o0 < T ? (uint32_t)(n - o0) : T;
    const uint64_t a0 = o0 / (2ull * run) * (2ull * run);  /* the pair of runs it lies in */
    const uint32_t na = n - a0 < run ? (uint32_t)(n - a0) : run;
    const uint64_t b0 = a0 + na;
    const uint32_t nb = n - b0 < run ? (uint32_t)(n - b0) : run;
    if (nb == 0) {
        for (uint32_t i = threadIdx.x; i < cnt; i += WG)
            out[o0 + i] = in[o0 + i];
        return;
    }
    const KeyLess lt{Keys{a.src, a.rb}};
    const uint32_t d0 = (uint32_t)(o0 - a0);
    if (threadIdx.x < 2)
        s_cut[threadIdx.x] = diag_search(in + a0, na, in + b0, nb, threadIdx.x ? d0 + cnt : d0, lt);
    __syncthreads();
    const uint32_t i0 = s_cut[0], ca = s_cut[1] - i0, cb = cnt - ca;
    const Entry *pa = in + a0 + i0, *pb = in + b0 + (d0 - i0);
    for (uint32_t i = threadIdx.x; i < cnt; i += WG)
        s[i] = i < ca ? pa[i] : pb[i - ca];
    __syncthreads();
    const uint32_t vt = (T + WG - 1) / WG, d = threadIdx.x * vt;
    if (d >= cnt)
        return;
    const Entry *sa = s, *sb = s + ca;
    uint32_t i = diag_search(sa, ca, sb, cb, d, lt), j = d - i;
    for (uint32_t v = 0; v < vt && d + v < cnt; ++v) {
        const bool take_a = j >= cb || (i < ca && !lt(sb[j], sa[i]));
        out[o0 + d + v] = take_a ? sa[i++] : sb[j++];
    }
}

__global__ __launch_bounds__(WG) void merge_flag_kernel(Merge a)
{
    __shared__ uint64_t s_part[WG / 64];
    if (is_bad(a))
        return;
    const Keys K{a.src, a.rb};
    const uint64_t first = (uint64_t)blockIdx.x * BLOCK_RECS;
    uint64_t winners = 0, deletes = 0, sumk = 0, sumv = 0, dropped = 0;
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k) {
        const uint64_t i = first + k * WG + threadIdx.x;
        if (i >= a.n)
            break;
        const int f = winner_flag(K, a.sorted, i, a.n, a.drop != 0);
        a.flags[i] = (uint8_t)f;
        if (f == F_WINNER) {
            const zscrc_zs_record r = a.rb[a.sorted[i].seq];
            ++winners;
            sumk += r.key_len;
            if (is_delete(r))
                ++deletes;
            else
                sumv += r.val_len;
        } else if (f == F_DROPPED) {
            ++dropped;
        }
    }
    winners = wg_sum(s_part, winners);
    deletes = wg_sum(s_part, deletes);
    sumk = wg_sum(s_part, sumk);
    sumv = wg_sum(s_part, sumv);
    dropped = wg_sum(s_part, dropped);
    if (threadIdx.x != 0)
        return;
    a.bcount[blockIdx.x] = (uint32_t)winners;
    if (deletes)
        atomicAdd(a.sc + SC_DELETES, (unsigned long long)deletes);
    if (sumk)
        atomicAdd(a.sc + SC_SUMK, (unsigned long long)sumk);
    if (sumv)
        atomicAdd(a.sc + SC_SUMV, (unsigned long long)sumv);
    if (dropped)
        atomicAdd(a.sc + SC_DROPPED, (unsigned long long)dropped);
}

__global__ __launch_bounds__(WG) void merge_scan_kernel(Merge a)
{
    __shared__ uint64_t s_scan[WG / 64];
    const uint64_t bad = a.n ? a.sc[SC_BAD] : U64_MAX;
    uint64_t carry = 0;
    if (bad == U64_MAX)
        carry = scan_counts(
            s_scan, a.nblocks, [&a](uint64_t i) { return (uint64_t)a.bcount[i]; },
            [&a](uint64_t i, uint64_t at) { a.bcount[i] = (uint32_t)at; });
    if (threadIdx.x != 0)
        return;
    if (bad != U64_MAX) {
        a.res[0] = (uint64_t)(int64_t)ZSCRC_EINVAL;
        a.res[1] = bad;
        a.res[2] = a.n;
        for (int i = 3; i < ZSCRC_MERGE_RES_WORDS; ++i)
            a.res[i] = 0;
        return;
    }
    const uint64_t dropped = a.n ? a.sc[SC_DROPPED] : 0;
    a.res[0] = carry > a.cap ? (uint64_t)ZSCRC_ZS_OVERFLOW : 0;
    a.res[1] = carry;
    a.res[2] = a.n;
    a.res[3] = a.n ? a.sc[SC_DELETES] : 0;
    a.res[4] = a.n ? a.sc[SC_SUMK] : 0;
    a.res[5] = a.n ? a.sc[SC_SUMV] : 0;
    a.res[6] = a.n - carry - dropped;
    a.res[7] = dropped;
}

__global__ __launch_bounds__(WG) void merge_scatter_kernel(Merge a)
{
    __shared__ uint64_t s_scan[WG / 64];
    if (is_bad(a))
        return;
    const uint64_t first = (uint64_t)blockIdx.x * BLOCK_RECS;
    uint64_t carry = a.bcount[blockIdx.x];
    if (carry >= a.cap)
        return;
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k) {
        const uint64_t i = first + k * WG + threadIdx.x;
        const bool win = i < a.n && a.flags[i] == F_WINNER;
        uint64_t total;
        const uint64_t at = carry + wg_scan(s_scan, win, total);
        if (win && at < a.cap)
            a.out[at] = a.rb[a.sorted[i].seq];
        carry += total;
    }
}

/* The tile of a call; 0 = a bad option. */
uint32_t tile_of(const zscrc_merge_opts *o)
{
    return (uint32_t)pow2_opt(o ? o->tile_records : 0, DEF_TILE, TILE_MIN, TILE_MAX);
}

/* The pieces of the scratch into a, each on a 16-byte boundary (at most min(n,
 * ZSCRC_WALK_MULTI_MAX) lists are not empty); the bytes. */
size_t carve(Merge &a, zs::Carve c)
{
    const size_t n = a.n, kmax = n < ZSCRC_WALK_MULTI_MAX ? n : ZSCRC_WALK_MULTI_MAX;
    a.nblocks = (uint32_t)blocks_of(n);
    a.sc = c.take<unsigned long long>(SC_WORDS, 16);
    a.lists = c.take<ListD>(kmax + 1, 16);
    a.rb = c.take<zscrc_zs_record>(n, 16);
    a.e0 = c.take<Entry>(n, 16);
    a.e1 = c.take<Entry>(n, 16);
    a.bcount = c.take<uint32_t>(a.nblocks + 1, 16);
    a.flags = c.take<uint8_t>(n, 16);
    return up16(c.bytes());
}

int launch(Merge &a, void *scratch, zs::Scratch &sc, const zscrc_merge_list *lists, size_t k, hipStream_t s)
{
    carve(a, zs::Carve(scratch));
    a.sorted = a.e0;
    if (a.n) {
        const int rc = stage_lists(sc, lists, k, a.k, a.lists, s);
        if (rc)
            return rc;
        if (hipMemsetAsync(a.sc, 0, SC_WORDS * 8, s) != hipSuccess ||
            hipMemsetAsync(a.sc + SC_BAD, 0xFF, 8, s) != hipSuccess)
            return ZSCRC_EHIP;
        const uint32_t T = a.tile, tiles = (a.n + T - 1) / T;
        hipLaunchKernelGGL(merge_gather_kernel, dim3((a.n + WG - 1) / WG), dim3(WG), 0, s, a);
        hipLaunchKernelGGL(merge_sort_kernel, dim3(tiles), dim3(WG), T * (sizeof(Entry) + 8), s, a);
        Entry *in = a.e0, *out = a.e1;
        for (uint64_t run = T; run < a.n; run *= 2) {
            hipLaunchKernelGGL(merge_pass_kernel, dim3(tiles), dim3(WG), T * sizeof(Entry), s, a, in, out,
                               (uint32_t)run);
            Entry *t = in;
            in = out;
            out = t;
        }
        a.sorted = in;
        hipLaunchKernelGGL(merge_flag_kernel, dim3(a.nblocks), dim3(WG), 0, s, a);
    }
    hipLaunchKernelGGL(merge_scan_kernel, dim3(1), dim3(WG), 0, s, a);
    if (a.n && a.cap)
        hipLaunchKernelGGL(merge_scatter_kernel, dim3(a.nblocks), dim3(WG), 0, s, a);
    return hipGetLastError() == hipSuccess ? ZSCRC_OK : ZSCRC_EHIP;
}

} /* namespace */

extern "C" {

size_t zscrc_device_merge_scratch_bytes(size_t n_total, const zscrc_merge_opts *opts)
{
    if (!tile_of(opts) || n_total > N_MAX)
        return 0;
    Merge a{};
    a.n = (uint32_t)n_total;
    return carve(a, zs::Carve(nullptr));
}

int zscrc_device_merge(const void *d_src, uint64_t src_size, const zscrc_merge_list *lists, size_t k,
                       struct zscrc_zs_record *d_out, size_t cap, uint64_t *d_res, void *scratch,
                       const zscrc_merge_opts *opts, unsigned flags, void *stream)
{
    const uint32_t tile = tile_of(opts);
    uint64_t n = 0;
    uint32_t filled = 0;
    if (!d_res || (!d_src && src_size) || (cap && !d_out) || (reinterpret_cast<uintptr_t>(scratch) & 15) ||
        (flags & ~ZSCRC_MERGE_DROP_DELETES) || !tile || src_size > zspack::SRC_MAX ||
        !lists_ok(lists, k, ZSCRC_WALK_MULTI_MAX, &n, &filled))
        return ZSCRC_EINVAL;
    Merge a{};
    a.src = static_cast<const uint8_t *>(d_src);
    a.src_size = src_size;
    a.k = filled;
    a.n = (uint32_t)n;
    a.tile = tile;
    a.drop = flags & ZSCRC_MERGE_DROP_DELETES;
    a.out = d_out;
    a.cap = cap;
    a.res = d_res;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return zs::with_scratch(scratch, carve(a, zs::Carve(nullptr)), true, s,
                            [&](void *sp, zs::Scratch *sc) { return launch(a, sp, *sc, lists, k, s); });
}

} /* extern "C" */
