/*
 * zscrc_devpack.hip -- the packed-file writer of zscrc_pack.cpp on the device:
 * zscrc_device_pack writes the byte-exact packed file of a device-resident
 * record list into device memory, CRCs included, with no image byte crossing
 * PCIe ("The packer on the device").  The layout arithmetic is
 * zscrc_pack_layout.h's, shared with the host.
 *
 * Launches, all in stream order, no workgroup waiting for another one:
 *
 *   pack_size_kernel    one workgroup per BLOCK_RECS records: every record
 *                       checked against the source (the smallest bad index by
 *                       an integer min) and the block's sum of serialised
 *                       lengths
 *   pack_scan_kernel    one workgroup: the block sums to their exclusive
 *                       prefix, the layout (region, commits short or long,
 *                       pointer section, file size), the result words [0..3],
 *                       the two spans to checksum as device descriptors and
 *                       the count that heads the pointer section
 *   pack_prefix_kernel  one workgroup per block: each record's start in the
 *                       region (8 bytes a record) and its big-endian pointer
 *   pack_copy_kernel    the hot path: the records region by the tile sweep
 *                       that the log writer shares (zscrc_copy_tiles.h)
 *   (the library's variable-length batch over the two span descriptors)
 *   pack_seal_kernel    one lane: the two commit records from the span CRCs,
 *                       the header, the result words [4..7]
 *
 * The host never learns the region's size: grids are sized from the record
 * count and the output's capacity, the kernels read the totals the scan left
 * on the device.  A result code other than 0 makes every later kernel return
 * at once, and the span descriptors empty.
 *
 * The sums and prefix sums are zscrc_wg.h's with its addition that saturates
 * (pack_scan_kernel: scan_counts); the scratch of a call comes through
 * zs::with_scratch (zscrc_internal.h, zscrc_scratch.cpp), laid out by carve();
 * the option rule, the pointer checks and the copy's grid: zsdev's, there too.
 */
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/zscrc.h"
#include "zscrc_copy_tiles.h"
#include "zscrc_internal.h"
#include "zscrc_pack_layout.h"
#include "zscrc_wg.h"

namespace {

using namespace zspack;
using namespace zsdev;
using namespace zstile;

/* scratch: SC_WORDS words, then nblocks + 1 block sums, then n + 1 starts */
enum { SC_BAD = 0, SC_CODE = 1, SC_REGION = 2, SC_PTR_OFF = 3, SC_DOFF = 4, SC_DLEN = 6, SC_CRC = 8, SC_WORDS = 16 };

struct Pack {
    const uint8_t *src;
    uint64_t src_size;
    const zscrc_zs_record *recs;
    uint64_t n;
    uint8_t *out;
    uint64_t out_cap;
    uint64_t *res;
    uint64_t *sc;     /* SC_WORDS words */
    uint64_t *bsum;   /* nblocks + 1 */
    uint64_t *start;  /* n + 1 */
    uint64_t nblocks;
    uint64_t tile;
};

/* The serialised length of record i, 0 past the list or for a bad record. */
__device__ inline uint64_t len_of(const Pack &a, uint64_t i, bool *bad)
{
    *bad = false;
    if (i >= a.n)
        return 0;
    const zscrc_zs_record r = a.recs[i];
    if (!rec_ok(r, a.src_size)) {
        *bad = true;
        return 0;
    }
    return rec_len(r);
}

__global__ __launch_bounds__(WG) void pack_size_kernel(Pack a)
{
    __shared__ uint64_t s_part[WG / 64];
    const uint64_t first = (uint64_t)blockIdx.x * BLOCK_RECS;
    uint64_t sum = 0, bad_at = U64_MAX;
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k) {
        const uint64_t i = first + k * WG + threadIdx.x;
        bool bad;
        sum = sat_add(sum, len_of(a, i, &bad));
        if (bad && i < bad_at)
            bad_at = i;
    }
    if (bad_at != U64_MAX)
        atomicMin(reinterpret_cast<unsigned long long *>(a.sc + SC_BAD), (unsigned long long)bad_at);
    sum = wg_sum(s_part, sum, SatAdd{});
    if (threadIdx.x == 0)
        a.bsum[blockIdx.x] = sum;
}

__global__ __launch_bounds__(WG) void pack_scan_kernel(Pack a)
{
    __shared__ uint64_t s_scan[WG / 64];
    const uint64_t carry = scan_counts(
        s_scan, a.nblocks, [&a](uint64_t i) { return a.bsum[i]; }, [&a](uint64_t i, uint64_t at) { a.bsum[i] = at; },
        SatAdd{});
    if (threadIdx.x != 0)
        return;
    const uint64_t bad = a.n ? a.sc[SC_BAD] : U64_MAX;
    const Layout l = layout(a.n, carry);
    const uint64_t code = bad != U64_MAX ? (uint64_t)(int64_t)ZSCRC_EINVAL
                                         : l.file_bytes > a.out_cap ? (uint64_t)ZSCRC_ZS_OVERFLOW : 0;
    a.res[0] = code;
    a.res[1] = bad != U64_MAX ? bad : a.n;
    a.res[2] = l.file_bytes;
    a.res[3] = l.region;
    for (int i = 4; i < ZSCRC_PACK_RES_WORDS; ++i)
        a.res[i] = 0;
    a.sc[SC_CODE] = code;
    a.sc[SC_REGION] = l.region;
    a.sc[SC_PTR_OFF] = l.ptr_off;
    /* the spans the batch checksums: records region, pointer section */
    a.sc[SC_DOFF] = code ? 0 : HDR;
    a.sc[SC_DOFF + 1] = code ? 0 : l.ptr_off;
    a.sc[SC_DLEN] = code ? 0 : l.region;
    a.sc[SC_DLEN + 1] = code ? 0 : l.ptr_bytes;
    a.sc[SC_CRC] = 0;
    a.bsum[a.nblocks] = l.region;
    a.start[a.n] = l.region;
    /* the count heads the pointer section and is part of its span */
    if (!code)
        *reinterpret_cast<uint64_t *>(a.out + l.ptr_off) = mem_be64(a.n);
}

__global__ __launch_bounds__(WG) void pack_prefix_kernel(Pack a)
{
    __shared__ uint64_t s_scan[WG / 64];
    if (a.sc[SC_CODE] != 0)
        return;
    uint64_t *ptrs = reinterpret_cast<uint64_t *>(a.out + a.sc[SC_PTR_OFF]) + 1;
    const uint64_t first = (uint64_t)blockIdx.x * BLOCK_RECS;
    uint64_t carry = a.bsum[blockIdx.x];
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k) {
        const uint64_t i = first + k * WG + threadIdx.x;
        bool bad;
        const uint64_t len = len_of(a, i, &bad);
        uint64_t total;
        const uint64_t at = carry + wg_scan(s_scan, len, total, SatAdd{});
        if (i < a.n) {
            a.start[i] = at;
            ptrs[i] = mem_be64(HDR + at);
        }
        carry += total;
    }
}

/* The records region [40, 40 + region) by zscrc_copy_tiles.h's sweep: the
 * starts are region coordinates, and the records fill the region. */
__global__ __launch_bounds__(WG) void pack_copy_kernel(Pack a)
{
    __shared__ uint64_t s_start[LDS_STARTS];
    if (a.sc[SC_CODE] != 0)
        return;
    const uint64_t region = a.sc[SC_REGION];
    if (region == 0)
        return;
    copy_tiles<HDR, false>(a.src, a.recs, a.start, a.n, a.out, a.tile, HDR, HDR + region, s_start);
}

__global__ __launch_bounds__(64) void pack_seal_kernel(Pack a, Header h)
{
    if (threadIdx.x != 0 || blockIdx.x != 0 || a.sc[SC_CODE] != 0)
        return;
    const uint64_t region = a.sc[SC_REGION], ptr_off = a.sc[SC_PTR_OFF], ptr_bytes = 8 * (a.n + 1);
    const uint32_t *crc = reinterpret_cast<const uint32_t *>(a.sc + SC_CRC);
    uint64_t *out = reinterpret_cast<uint64_t *>(a.out);
    uint64_t w[3];
    uint32_t commit_crc, final_crc;
    int k = commit_words(crc[0], region, false, w, &commit_crc);
    for (int i = 0; i < k; ++i)
        out[(HDR + region) / 8 + i] = w[i];
    k = commit_words(crc[1], ptr_bytes, true, w, &final_crc);
    for (int i = 0; i < k; ++i)
        out[(ptr_off + ptr_bytes) / 8 + i] = w[i];
    for (int i = 0; i < 5; ++i)
        out[i] = h.w[i];
    a.res[4] = crc[0];
    a.res[5] = crc[1];
    a.res[6] = commit_crc;
    a.res[7] = final_crc;
}

/* The tile of a call; 0 = a bad option. */
uint64_t tile_of(const zscrc_pack_opts *o) { return pow2_opt(o ? o->tile_bytes : 0, DEF_TILE, TILE_MIN, TILE_MAX); }

/* The pieces of the scratch into a, one 8-byte array behind the other; the bytes. */
size_t carve(Pack &a, zs::Carve c)
{
    a.nblocks = blocks_of(a.n);
    a.sc = c.take<uint64_t>(SC_WORDS, 16);
    a.bsum = c.take<uint64_t>(a.nblocks + 1);
    a.start = c.take<uint64_t>(a.n + 1);
    return up16(c.bytes());
}

int launch(Pack &a, void *scratch, const Header &h, hipStream_t s)
{
    carve(a, zs::Carve(scratch));
    if (a.n) {
        if (hipMemsetAsync(a.sc + SC_BAD, 0xFF, 8, s) != hipSuccess)
            return ZSCRC_EHIP;
        hipLaunchKernelGGL(pack_size_kernel, dim3((unsigned)a.nblocks), dim3(WG), 0, s, a);
    }
    hipLaunchKernelGGL(pack_scan_kernel, dim3(1), dim3(WG), 0, s, a);
    if (hipGetLastError() != hipSuccess)
        return ZSCRC_EHIP;
    /* no file fits fewer than 64 bytes: the sizing call ends here */
    if (a.out_cap < 64)
        return ZSCRC_OK;
    if (a.n) {
        /* the region's size is on the device only */
        unsigned g;
        if (copy_grid(a.out_cap, a.tile, COPY_WG_PER_CU, &g) != ZSCRC_OK)
            return ZSCRC_EHIP;
        hipLaunchKernelGGL(pack_prefix_kernel, dim3((unsigned)a.nblocks), dim3(WG), 0, s, a);
        hipLaunchKernelGGL(pack_copy_kernel, dim3(g), dim3(WG), 0, s, a);
    }
    if (hipGetLastError() != hipSuccess)
        return ZSCRC_EHIP;
    const int rc = zscrc_device_batch(a.out, a.sc + SC_DOFF, a.sc + SC_DLEN, nullptr,
                                      reinterpret_cast<uint32_t *>(a.sc + SC_CRC), 2, 0, s);
    if (rc)
        return rc;
    hipLaunchKernelGGL(pack_seal_kernel, dim3(1), dim3(64), 0, s, a, h);
    return hipGetLastError() == hipSuccess ? ZSCRC_OK : ZSCRC_EHIP;
}

} /* namespace */

extern "C" {

uint64_t zscrc_device_pack_bound(uint64_t n, uint64_t sum_key_len, uint64_t sum_val_len)
{
    uint64_t b;
    if (__builtin_mul_overflow(n, (uint64_t)62, &b) || __builtin_add_overflow(b, (uint64_t)120, &b) ||
        __builtin_add_overflow(b, sum_key_len, &b) || __builtin_add_overflow(b, sum_val_len, &b))
        return 0;
    return b;
}

size_t zscrc_device_pack_scratch_bytes(size_t n, const zscrc_pack_opts *opts)
{
    if (!tile_of(opts) || n > N_MAX)
        return 0;
    Pack a{};
    a.n = n;
    return carve(a, zs::Carve(nullptr));
}

int zscrc_device_pack(const void *d_src, uint64_t src_size, const struct zscrc_zs_record *d_recs, size_t n,
                      const uint8_t uuid[16], uint32_t startidx, uint32_t endidx, void *d_out, uint64_t out_cap,
                      uint64_t *d_res, void *scratch, const zscrc_pack_opts *opts, unsigned flags, void *stream)
{
    const uint64_t tile = tile_of(opts);
    if (!d_res || !uuid || (n && !d_recs) || (reinterpret_cast<uintptr_t>(scratch) & 15) || flags || !tile ||
        n > N_MAX || src_size > SRC_MAX || !src_out_ok(d_src, src_size, d_out, out_cap, true))
        return ZSCRC_EINVAL;
    Pack a{};
    a.src = static_cast<const uint8_t *>(d_src);
    a.src_size = src_size;
    a.recs = d_recs;
    a.n = n;
    a.out = static_cast<uint8_t *>(d_out);
    a.out_cap = out_cap;
    a.res = d_res;
    a.tile = tile;
    const Header h = header_words(uuid, startidx, endidx);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return zs::with_scratch(scratch, carve(a, zs::Carve(nullptr)), false, s,
                            [&](void *p, zs::Scratch *) { return launch(a, p, h, s); });
}

} /* extern "C" */
