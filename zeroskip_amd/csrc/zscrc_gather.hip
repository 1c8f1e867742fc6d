/*
 * zscrc_gather.hip -- the second half of the read path for stores that live in
 * device memory: zscrc_device_gather copies the values a batch of hits (or a
 * record list) names out of d_src into one dense buffer, with the CSR offsets
 * of the values and, if asked, their CRCs, no byte crossing PCIe (DESIGN.md
 * 2.6, "The value gather on the device"); zscrc_zs_gather is the same gather
 * in host memory.  The arithmetic is zscrc_gather_layout.h's, shared with the
 * host.
 *
 * Launches, all in stream order, no workgroup waiting for another one:
 *
 *   gather_size_kernel    one workgroup per BLOCK_RECS items: every item
 *                         classified, a value checked against the source (the
 *                         smallest bad index by an integer min), the block's
 *                         saturating sum of lengths, the counts of the four
 *                         kinds by integer adds, the longest value by an
 *                         integer max
 *   gather_scan_kernel    one workgroup: the block sums to their exclusive
 *                         prefix, the code, the result words, offs[nq]
 *   gather_prefix_kernel  one workgroup per block: offs[i], and for the CRC
 *                         batch each value's offset and length (all zero on a
 *                         code other than 0)
 *   gather_copy_kernel    the hot path: the output is cut into 16-byte aligned
 *                         tiles, a workgroup takes a run of consecutive tiles
 *                         and works through it in chunks: the next STAGE + 1
 *                         starts from offs into LDS, then every thread builds
 *                         whole aligned 16-byte output words of the chunk out
 *                         of source bytes gathered from any alignment.  A
 *                         chunk ends at the tile's end or with the staged
 *                         starts, and the run goes on from there: the LDS is
 *                         fixed, however many items reach into a tile
 *   (the library's variable-length batch over the gathered values)
 *
 * The host never learns the total: grids are sized from nq and the output's
 * capacity, the kernels read the code and the total the scan left on the
 * device.  The copy writes the bytes [0, total) of the output and no other:
 * the last word, where the total is no multiple of 16, is an 8-byte store of
 * its first half if that is whole and byte stores of the rest -- so the bound
 * of its writes is the total itself, below both the total rounded up to 16
 * and out_cap.
 *
 * The sums are zscrc_wg.h's; the scratch is laid out by carve(); the option
 * rule, the pointer checks and the copy's grid are zsdev's (zscrc_internal.h).
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "../../include/zscrc.h"
#include "zscrc_gather_layout.h"
#include "zscrc_internal.h"
#include "zscrc_wg.h"

extern "C" uint32_t zscrc_cpu_hw(uint32_t crc, const void *buf, size_t len);

namespace {

using namespace zsgather;
using namespace zsdev;
using zspack::find_rec;

/* the default: measured, DESIGN.md 2.6 */
constexpr uint64_t DEF_TILE = 16384, TILE_MIN = 64, TILE_MAX = 65536;
/* starts a chunk stages in LDS, in rounds of WG loads; the last one staged
 * ends the chunk, so a chunk holds STAGE - 1 items at the most */
constexpr uint32_t STAGE = 1024;
/* 8 KiB of starts: the eight workgroups of 256 threads a CU holds are all
 * resident, so the equal runs of tiles end together */
constexpr unsigned COPY_WG_PER_CU = 8;

/* scratch: SC_WORDS words, then nblocks + 1 block sums, then for the CRC
 * batch nq lengths and nq offsets */
enum { SC_BAD = 0, SC_CODE = 1, SC_TOTAL = 2, SC_KIND = 8, SC_LONGEST = 12, SC_WORDS = 16 };

struct Item {
    uint64_t w0, w1, val_off, val_len;
};

struct Gather {
    const uint8_t *src;
    uint64_t src_size;
    const Item *items;
    uint64_t nq;
    uint8_t *out;
    uint64_t out_cap;
    uint64_t *offs;   /* nq + 1 */
    uint64_t *res;
    unsigned long long *sc; /* SC_WORDS words */
    uint64_t *bsum;   /* nblocks + 1 */
    uint64_t *clen;   /* nq, or NULL: no CRCs */
    uint64_t *coff;   /* nq */
    uint64_t nblocks;
    uint64_t tile;
};

struct Max {
    __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return a > b ? a : b; }
};

/* Item i: its kind and the bytes it adds; *bad: a value outside the source. */
__device__ inline uint64_t item_len(const Gather &a, uint64_t i, Kind *k, bool *bad)
{
    const Item it = a.items[i];
    *k = kind_of(it.w0, it.val_off);
    *bad = *k == VALUE && !value_ok(it.val_off, it.val_len, a.src_size);
    return *bad ? 0 : len_of(*k, it.val_len);
}

__global__ __launch_bounds__(WG) void gather_size_kernel(Gather a)
{
    __shared__ uint64_t s_part[WG / 64];
    const uint64_t first = (uint64_t)blockIdx.x * BLOCK_RECS;
    uint64_t sum = 0, bad_at = U64_MAX, longest = 0, kinds[KINDS] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k) {
        const uint64_t i = first + k * WG + threadIdx.x;
        if (i >= a.nq)
            continue;
        Kind kind;
        bool bad;
        const uint64_t len = item_len(a, i, &kind, &bad);
        if (bad && i < bad_at)
            bad_at = i;
        sum = sum_len(sum, len);
        longest = len > longest ? len : longest;
#pragma unroll
        for (int c = 0; c < KINDS; ++c)
            kinds[c] += kind == c;
    }
    if (bad_at != U64_MAX)
        atomicMin(a.sc + SC_BAD, (unsigned long long)bad_at);
    sum = wg_sum(s_part, sum, SatAdd{});
    longest = wg_sum(s_part, longest, Max{});
#pragma unroll
    for (int c = 0; c < KINDS; ++c)
        kinds[c] = wg_sum(s_part, kinds[c]);
    if (threadIdx.x != 0)
        return;
    a.bsum[blockIdx.x] = sum;
#pragma unroll
    for (int c = 0; c < KINDS; ++c)
        if (kinds[c])
            atomicAdd(a.sc + SC_KIND + c, (unsigned long long)kinds[c]);
    if (longest)
        atomicMax(a.sc + SC_LONGEST, (unsigned long long)longest);
}

__global__ __launch_bounds__(WG) void gather_scan_kernel(Gather a)
{
    __shared__ uint64_t s_scan[WG / 64];
    const uint64_t total = scan_counts(
        s_scan, a.nblocks, [&a](uint64_t i) { return a.bsum[i]; }, [&a](uint64_t i, uint64_t at) { a.bsum[i] = at; },
        SatAdd{});
    if (threadIdx.x != 0)
        return;
    const uint64_t bad = a.nq ? a.sc[SC_BAD] : U64_MAX;
    const bool inval = bad != U64_MAX;
    const uint64_t code = inval ? (uint64_t)(int64_t)ZSCRC_EINVAL : total > a.out_cap ? (uint64_t)ZSCRC_ZS_OVERFLOW : 0;
    a.res[0] = code;
    a.res[1] = inval ? bad : a.nq;
    a.res[2] = inval || !a.nq ? 0 : a.sc[SC_KIND + VALUE];
    a.res[3] = inval ? 0 : total;
    a.res[4] = inval || !a.nq ? 0 : a.sc[SC_KIND + DELETED];
    a.res[5] = inval || !a.nq ? 0 : a.sc[SC_KIND + NOT_FOUND];
    a.res[6] = inval || !a.nq ? 0 : a.sc[SC_KIND + BAD_QUERY];
    a.res[7] = inval || !a.nq ? 0 : a.sc[SC_LONGEST];
    a.sc[SC_CODE] = code;
    a.sc[SC_TOTAL] = total;
    a.bsum[a.nblocks] = total;
    if (!inval)
        a.offs[a.nq] = total;
}

__global__ __launch_bounds__(WG) void gather_prefix_kernel(Gather a)
{
    __shared__ uint64_t s_scan[WG / 64];
    const uint64_t code = a.sc[SC_CODE];
    const bool inval = code == (uint64_t)(int64_t)ZSCRC_EINVAL;
    const uint64_t first = (uint64_t)blockIdx.x * BLOCK_RECS;
    uint64_t carry = a.bsum[blockIdx.x];
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k) {
        const uint64_t i = first + k * WG + threadIdx.x;
        Kind kind;
        bool bad;
        const uint64_t len = i < a.nq ? item_len(a, i, &kind, &bad) : 0;
        uint64_t total;
        const uint64_t at = sum_len(carry, wg_scan(s_scan, len, total, SatAdd{}));
        if (i < a.nq) {
            if (!inval)
                a.offs[i] = at;
            if (a.clen) {
                a.clen[i] = code ? 0 : len;
                a.coff[i] = code ? 0 : at;
            }
        }
        carry = sum_len(carry, total);
    }
}

/* The starts of a chunk's items from LDS, those past the staged ones from offs. */
struct ChunkOffs {
    const uint64_t *s, *g;
    uint64_t rec0;
    uint32_t m;
    __device__ uint64_t operator[](uint64_t i) const { return i - rec0 <= m ? s[i - rec0] : g[i]; }
};
struct ItemOffs {
    const Item *items;
    __device__ uint64_t operator()(uint64_t i) const { return items[i].val_off; }
};

/* The first n (1..16) bytes of the word (v0, v1) to the 16-byte aligned p: one
 * 16-byte store, or for the total's last word an 8-byte store of its first
 * half if that is whole and byte stores of the rest. */
__device__ inline void store_word(uint8_t *p, uint64_t v0, uint64_t v1, uint32_t n)
{
    if (n == 16) {
        u64x2 v;
        v.x = v0;
        v.y = v1;
        *reinterpret_cast<u64x2 *>(p) = v;
        return;
    }
    uint32_t b = 0;
    if (n >= 8) {
        *reinterpret_cast<uint64_t *>(p) = v0;
        b = 8;
    }
    for (; b < n; ++b)
        p[b] = (uint8_t)((b < 8 ? v0 : v1) >> (8 * (b & 7)));
}

/* The copy without the stage: every word's first item by bisection of offs in
 * global memory, no LDS.  Measured against the staged chunks and slower
 * (DESIGN.md 2.6); ZSCRC_GATHER_SEARCH=1 in the environment selects it. */
__global__ __launch_bounds__(WG) void gather_copy_search_kernel(Gather a)
{
    if (a.sc[SC_CODE] != 0)
        return;
    const uint64_t total = a.sc[SC_TOTAL];
    const ItemOffs val_off{a.items};
    const uint64_t *offs = a.offs;
    const uint64_t stride = (uint64_t)gridDim.x * WG * 16;
    for (uint64_t f = ((uint64_t)blockIdx.x * WG + threadIdx.x) * 16; f < total; f += stride) {
        uint64_t j = find_rec(offs, a.nq, f);
        const uint32_t n = total - f < 16 ? (uint32_t)(total - f) : 16;
        const uint64_t v0 = build8(a.src, offs, val_off, j, f, n < 8 ? n : 8);
        const uint64_t v1 = n > 8 ? build8(a.src, offs, val_off, j, f + 8, n - 8) : 0;
        store_word(a.out + f, v0, v1, n);
    }
}

__global__ __launch_bounds__(WG) void gather_copy_kernel(Gather a)
{
    __shared__ uint64_t s_start[STAGE];
    if (a.sc[SC_CODE] != 0)
        return;
    const uint64_t total = a.sc[SC_TOTAL];
    if (total == 0)
        return;
    const uint64_t T = a.tile, ntiles = (total + T - 1) / T;
    const uint64_t per = (ntiles + gridDim.x - 1) / gridDim.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * per;
    const uint64_t t1 = t0 + per < ntiles ? t0 + per : ntiles;
    if (t0 >= t1)
        return;
    const uint64_t end = t1 * T < total ? t1 * T : total;
    uint64_t lo = t0 * T;
    /* the item that holds the run's first byte: the largest one that starts
     * at or before it, so never one without bytes */
    uint64_t rec0 = find_rec(a.offs, a.nq, lo);
    const ItemOffs val_off{a.items};
    while (lo < end) {
        const uint64_t tile_end = (lo / T + 1) * T, hi = tile_end < end ? tile_end : end;
        /* s_start[j] = offs[rec0 + j], in rounds, up to a round that reaches hi (offs[nq] = total does) */
        uint32_t cnt = 0;
        for (uint32_t base = 0; base < STAGE; base += WG) {
            const uint64_t idx = rec0 + base + threadIdx.x;
            const uint64_t s = a.offs[idx < a.nq ? idx : a.nq];
            s_start[base + threadIdx.x] = s;
            cnt = base + WG;
            if ((uint32_t)__syncthreads_count(s < hi) < WG)
                break;
        }
        /* the chunk: the words that start below the last staged start, so the
         * item of a word's first byte is among the m staged ones with their ends */
        const uint32_t m = cnt - 1;
        const uint64_t staged = (s_start[m] + 15) & ~15ull, chi = staged < hi ? staged : hi;
        const ChunkOffs offs{s_start, a.offs, rec0, m};
        for (uint64_t f = lo + 16 * threadIdx.x; f < chi; f += 16 * WG) {
            uint64_t j = rec0 + find_rec(s_start, m, f);
            const uint32_t n = total - f < 16 ? (uint32_t)(total - f) : 16;
            const uint64_t v0 = build8(a.src, offs, val_off, j, f, n < 8 ? n : 8);
            const uint64_t v1 = n > 8 ? build8(a.src, offs, val_off, j, f + 8, n - 8) : 0;
            store_word(a.out + f, v0, v1, n);
        }
        /* the run goes on at next: in the last staged item that starts at or
         * before it (no words at all: every staged item lies before lo) */
        const uint64_t next = chi > lo ? chi : lo;
        const uint64_t adv = find_rec(s_start, (uint64_t)m + 1, next);
        __syncthreads(); /* s_start is rewritten by the next chunk */
        rec0 += adv;
        lo = next;
    }
}

/* The tile of a call; 0 = a bad option. */
uint64_t tile_of(const zscrc_gather_opts *o) { return pow2_opt(o ? o->tile_bytes : 0, DEF_TILE, TILE_MIN, TILE_MAX); }

/* The pieces of the scratch into a, one 8-byte array behind the other; the bytes. */
size_t carve(Gather &a, zs::Carve c)
{
    a.nblocks = blocks_of(a.nq);
    a.sc = c.take<unsigned long long>(SC_WORDS, 16);
    a.bsum = c.take<uint64_t>(a.nblocks + 1);
    a.clen = c.take<uint64_t>(a.nq);
    a.coff = c.take<uint64_t>(a.nq);
    return up16(c.bytes());
}

int launch(Gather &a, void *scratch, uint32_t *d_crcs, hipStream_t s)
{
    carve(a, zs::Carve(scratch));
    const bool sizing = !a.out && !a.out_cap;
    const bool crcs = d_crcs && !sizing && a.nq;
    if (!crcs)
        a.clen = a.coff = nullptr;
    if (a.nq) {
        if (hipMemsetAsync(a.sc + SC_BAD, 0xFF, 8, s) != hipSuccess ||
            hipMemsetAsync(a.sc + SC_KIND, 0, (SC_WORDS - SC_KIND) * 8, s) != hipSuccess)
            return ZSCRC_EHIP;
        hipLaunchKernelGGL(gather_size_kernel, dim3((unsigned)a.nblocks), dim3(WG), 0, s, a);
    }
    hipLaunchKernelGGL(gather_scan_kernel, dim3(1), dim3(WG), 0, s, a);
    if (a.nq)
        hipLaunchKernelGGL(gather_prefix_kernel, dim3((unsigned)a.nblocks), dim3(WG), 0, s, a);
    if (hipGetLastError() != hipSuccess)
        return ZSCRC_EHIP;
    if (a.nq && a.out_cap) {
        /* the total is on the device only */
        unsigned g;
        if (copy_grid(a.out_cap, a.tile, COPY_WG_PER_CU, &g) != ZSCRC_OK)
            return ZSCRC_EHIP;
        const char *search = getenv("ZSCRC_GATHER_SEARCH");
        if (search && search[0] == '1')
            hipLaunchKernelGGL(gather_copy_search_kernel, dim3(g), dim3(WG), 0, s, a);
        else
            hipLaunchKernelGGL(gather_copy_kernel, dim3(g), dim3(WG), 0, s, a);
        if (hipGetLastError() != hipSuccess)
            return ZSCRC_EHIP;
    }
    if (!crcs)
        return ZSCRC_OK;
    /* over the gathered bytes, so a CRC checks the copy end to end; on a code
     * other than 0 every descriptor is (0, 0) and every CRC 0 */
    return zscrc_device_batch(a.out, a.coff, a.clen, nullptr, d_crcs, a.nq, 0, s);
}

} /* namespace */

extern "C" {

size_t zscrc_device_gather_scratch_bytes(size_t nq, const zscrc_gather_opts *opts)
{
    if (!tile_of(opts) || nq > N_MAX)
        return 0;
    Gather a{};
    a.nq = nq;
    return carve(a, zs::Carve(nullptr));
}

int zscrc_device_gather(const void *d_src, uint64_t src_size, const zscrc_find_hit *d_items, size_t nq, void *d_out,
                        uint64_t out_cap, uint64_t *d_offs, uint32_t *d_crcs, uint64_t *d_res, void *scratch,
                        const zscrc_gather_opts *opts, unsigned flags, void *stream)
{
    static_assert(sizeof(Item) == sizeof(zscrc_find_hit) && sizeof(Item) == sizeof(zscrc_zs_record),
                  "an item is four words");
    const uint64_t tile = tile_of(opts);
    if (!d_res || !d_offs || (nq && !d_items) || (reinterpret_cast<uintptr_t>(scratch) & 15) || flags || !tile ||
        nq > N_MAX || src_size > zspack::SRC_MAX || !src_out_ok(d_src, src_size, d_out, out_cap, true))
        return ZSCRC_EINVAL;
    Gather a{};
    a.src = static_cast<const uint8_t *>(d_src);
    a.src_size = src_size;
    a.items = reinterpret_cast<const Item *>(d_items);
    a.nq = nq;
    a.out = static_cast<uint8_t *>(d_out);
    a.out_cap = out_cap;
    a.offs = d_offs;
    a.res = d_res;
    a.tile = tile;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return zs::with_scratch(scratch, carve(a, zs::Carve(nullptr)), false, s,
                            [&](void *p, zs::Scratch *) { return launch(a, p, d_crcs, s); });
}

int zscrc_zs_gather(const void *src, uint64_t src_size, const zscrc_find_hit *items, size_t nq, void *out,
                    uint64_t out_cap, uint64_t *offs, uint32_t *crcs, uint64_t res[ZSCRC_GATHER_RES_WORDS])
{
    if (!res || !offs || (nq && !items) || nq > N_MAX || src_size > zspack::SRC_MAX ||
        !src_out_ok(src, src_size, out, out_cap, false))
        return ZSCRC_EINVAL;
    const uint8_t *s = static_cast<const uint8_t *>(src);
    uint8_t *o = static_cast<uint8_t *>(out);
    const Item *it = reinterpret_cast<const Item *>(items);
    const bool sizing = !out && !out_cap;
    memset(res, 0, ZSCRC_GATHER_RES_WORDS * 8);
    /* size: the kinds, the check, the total */
    uint64_t total = 0, kinds[KINDS] = {0, 0, 0, 0}, longest = 0;
    for (size_t i = 0; i < nq; ++i) {
        const Kind k = kind_of(it[i].w0, it[i].val_off);
        if (k == VALUE && !value_ok(it[i].val_off, it[i].val_len, src_size)) {
            res[0] = (uint64_t)(int64_t)ZSCRC_EINVAL;
            res[1] = i;
            if (crcs && !sizing)
                memset(crcs, 0, nq * 4);
            return ZSCRC_OK;
        }
        const uint64_t len = len_of(k, it[i].val_len);
        ++kinds[k];
        total = sum_len(total, len);
        longest = len > longest ? len : longest;
    }
    /* prefix */
    uint64_t at = 0;
    for (size_t i = 0; i < nq; ++i) {
        offs[i] = at;
        at = sum_len(at, len_of(kind_of(it[i].w0, it[i].val_off), it[i].val_len));
    }
    offs[nq] = total;
    res[0] = total > out_cap ? ZSCRC_ZS_OVERFLOW : 0;
    res[1] = nq;
    res[2] = kinds[VALUE];
    res[3] = total;
    res[4] = kinds[DELETED];
    res[5] = kinds[NOT_FOUND];
    res[6] = kinds[BAD_QUERY];
    res[7] = longest;
    if (res[0]) {
        if (crcs && !sizing)
            memset(crcs, 0, nq * 4);
        return ZSCRC_OK;
    }
    /* copy: the words the kernel builds, eight bytes at a time */
    uint64_t j = 0;
    const auto val_off = [it](uint64_t i) { return it[i].val_off; };
    for (uint64_t p = 0; p < total; p += 8) {
        const uint32_t n = total - p < 8 ? (uint32_t)(total - p) : 8;
        const uint64_t v = build8(s, offs, val_off, j, p, n);
        memcpy(o + p, &v, n);
    }
    if (crcs && !sizing)
        for (size_t i = 0; i < nq; ++i)
            crcs[i] = offs[i + 1] > offs[i] ? zscrc_cpu_hw(0, o + offs[i], (size_t)(offs[i + 1] - offs[i])) : 0;
    return ZSCRC_OK;
}

} /* extern "C" */
