/*
 * zscrc_devlog.hip -- the log writer on the device: zscrc_device_log writes
 * what zsdb_add / zsdb_remove / zsdb_commit append to an active file, for a
 * record list and a transaction table that live in device memory, CRCs
 * included, with no byte crossing PCIe ("The log writer on the
 * device").  The layout arithmetic is zscrc_log_layout.h's and
 * zscrc_pack_layout.h's, shared with the host twin (zscrc_log.cpp).
 *
 * Launches, all in stream order, no workgroup waiting for another one:
 *
 *   log_size_kernel     one workgroup per BLOCK_RECS records: every record
 *                       checked (the smallest bad index by an integer min), the
 *                       block's sum of serialised lengths and its largest
 *                       delete mark
 *   log_scan_kernel     one workgroup: both to their exclusive prefixes (the
 *                       sum saturates, the marks combine by max)
 *   log_prefix_kernel   one workgroup per block: P[i], the bytes before record
 *                       i, and D[i], the largest delete mark of records 0..i
 *   log_tx_kernel       one thread per transaction: the table checked (the
 *                       smallest bad entry by an integer min), the span's first
 *                       record and length, the block's sum of commit lengths
 *   log_txscan_kernel   one workgroup: the block sums to their prefix, the end
 *                       offset, the code and the result words [0..7]
 *   log_place_kernel    one thread per transaction: C[t], the commit bytes
 *                       before it, and the span descriptors in file offsets
 *   log_starts_kernel   one thread per record: its start P[i] + C[tx_of(i)] in
 *                       the file (in place of P[i]) and its listed entry
 *   log_copy_kernel     the hot path: the records by the tile sweep that the
 *                       packer shares (zscrc_copy_tiles.h); the words of
 *                       commit records are left to the seal
 *   (the library's variable-length batch over the span descriptors)
 *   log_seal_kernel     one thread per commit: its record from the span's CRC,
 *                       the finalise commit, the header, the result words
 *
 * Every grid is sized on the host from n, n_tx and the output's capacity; the
 * totals stay on the device.  A result code other than 0 makes every later
 * kernel return at once, and the span descriptors empty.
 */
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/zscrc.h"
#include "zscrc_copy_tiles.h"
#include "zscrc_internal.h"
#include "zscrc_log_layout.h"
#include "zscrc_wg.h"

namespace {

using namespace zspack;
using namespace zsdev;
using namespace zstile;

enum { SC_BAD = 0, SC_BADTX = 1, SC_CODE = 2, SC_BODY_END = 3, SC_WORDS = 8 };

/* Delete marks combine by max (identity 0), as wg_scan asks of an addition. */
struct MarkMax {
    __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return zslog::mark_max(a, b); }
};

struct Log {
    const uint8_t *src;
    uint64_t src_size;
    const zscrc_zs_record *recs;
    uint64_t n;
    const uint64_t *tx_end; /* NULL: one transaction a record */
    uint64_t ntx;           /* transactions */
    uint8_t *out;
    uint64_t out_cap, at;
    zscrc_zs_record *new_recs;
    uint64_t *span_off, *span_len; /* the caller's, may be NULL */
    uint64_t *res;
    uint64_t *sc;     /* SC_WORDS words */
    uint64_t *bsum;   /* nblocks + 1: bytes of the blocks before */
    uint64_t *bdel;   /* nblocks + 1: largest delete mark of the blocks before */
    uint64_t *start;  /* n + 1: P[i], then the record's file offset */
    uint64_t *tsum;   /* tblocks + 1: commit bytes of the transaction blocks before */
    uint64_t *cpre;   /* ntx: C[t] */
    uint64_t *sp_off; /* ntx + 1 span descriptors: P[first], then the file offset */
    uint64_t *sp_len;
    uint32_t *dmark;  /* n: D[i] */
    uint32_t *crc;    /* ntx + 1 span CRCs */
    uint64_t nblocks, tblocks;
    uint64_t tile;
    uint32_t prev_crc;
    uint32_t finalise;
};

/* Length and delete mark of record i; both 0 past the list or for a bad record. */
__device__ inline uint64_t len_of(const Log &a, uint64_t i, uint64_t *mark, bool *bad)
{
    *bad = false;
    *mark = 0;
    if (i >= a.n)
        return 0;
    const zscrc_zs_record r = a.recs[i];
    if (zslog::rec_bad(r, a.src_size)) {
        *bad = true;
        return 0;
    }
    *mark = zslog::del_mark(r, i);
    return rec_len(r);
}

__global__ __launch_bounds__(WG) void log_size_kernel(Log a)
{
    __shared__ uint64_t s_part[WG / 64];
    const uint64_t first = (uint64_t)blockIdx.x * BLOCK_RECS;
    uint64_t sum = 0, top = 0, bad_at = U64_MAX;
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k) {
        const uint64_t i = first + k * WG + threadIdx.x;
        uint64_t mark;
        bool bad;
        sum = sat_add(sum, len_of(a, i, &mark, &bad));
        top = zslog::mark_max(top, mark);
        if (bad && i < bad_at)
            bad_at = i;
    }
    if (bad_at != U64_MAX)
        atomicMin(reinterpret_cast<unsigned long long *>(a.sc + SC_BAD), (unsigned long long)bad_at);
    sum = wg_sum(s_part, sum, SatAdd{});
    top = wg_sum(s_part, top, MarkMax{});
    if (threadIdx.x == 0) {
        a.bsum[blockIdx.x] = sum;
        a.bdel[blockIdx.x] = top;
    }
}

__global__ __launch_bounds__(WG) void log_scan_kernel(Log a)
{
    __shared__ uint64_t s_scan[WG / 64];
    const uint64_t total = scan_counts(
        s_scan, a.nblocks, [&a](uint64_t i) { return a.bsum[i]; }, [&a](uint64_t i, uint64_t at) { a.bsum[i] = at; },
        SatAdd{});
    (void)scan_counts(
        s_scan, a.nblocks, [&a](uint64_t i) { return a.bdel[i]; }, [&a](uint64_t i, uint64_t at) { a.bdel[i] = at; },
        MarkMax{});
    if (threadIdx.x == 0) {
        a.bsum[a.nblocks] = total;
        a.start[a.n] = total; /* P[n] */
    }
}

__global__ __launch_bounds__(WG) void log_prefix_kernel(Log a)
{
    __shared__ uint64_t s_scan[WG / 64];
    const uint64_t first = (uint64_t)blockIdx.x * BLOCK_RECS;
    uint64_t carry = a.bsum[blockIdx.x], dcarry = a.bdel[blockIdx.x];
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k) {
        const uint64_t i = first + k * WG + threadIdx.x;
        uint64_t mark, total, dtotal;
        bool bad;
        const uint64_t len = len_of(a, i, &mark, &bad);
        const uint64_t at = sat_add(carry, wg_scan(s_scan, len, total, SatAdd{}));
        const uint64_t before = zslog::mark_max(dcarry, wg_scan(s_scan, mark, dtotal, MarkMax{}));
        if (i < a.n) {
            a.start[i] = at;
            a.dmark[i] = (uint32_t)zslog::mark_max(before, mark);
        }
        carry = sat_add(carry, total);
        dcarry = zslog::mark_max(dcarry, dtotal);
    }
}

/* The span of transaction t from P and D; its commit's length.  0 and *ok =
 * false for an entry of the table that is out of order. */
__device__ inline uint64_t tx_commit_len(const Log &a, uint64_t t, bool *ok)
{
    const uint64_t b = zslog::tx_begin(a.tx_end, t), e = zslog::tx_stop(a.tx_end, t);
    *ok = zslog::tx_ok(b, e, t, a.ntx, a.n);
    if (!*ok)
        return 0;
    const uint64_t s = zslog::span_first(b, e, e > b ? a.dmark[e - 1] : 0);
    const uint64_t p = a.start[s], len = zslog::span_bytes(p, a.start[e]);
    a.sp_off[t] = p;
    a.sp_len[t] = len;
    return commit_len(len);
}

__global__ __launch_bounds__(WG) void log_tx_kernel(Log a)
{
    __shared__ uint64_t s_part[WG / 64];
    const uint64_t first = (uint64_t)blockIdx.x * BLOCK_RECS;
    uint64_t sum = 0, bad_at = U64_MAX;
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k) {
        const uint64_t t = first + k * WG + threadIdx.x;
        if (t >= a.ntx)
            continue;
        bool ok;
        sum += tx_commit_len(a, t, &ok);
        if (!ok && t < bad_at)
            bad_at = t;
    }
    if (bad_at != U64_MAX)
        atomicMin(reinterpret_cast<unsigned long long *>(a.sc + SC_BADTX), (unsigned long long)bad_at);
    sum = wg_sum(s_part, sum);
    if (threadIdx.x == 0)
        a.tsum[blockIdx.x] = sum;
}

__global__ __launch_bounds__(WG) void log_txscan_kernel(Log a)
{
    __shared__ uint64_t s_scan[WG / 64];
    const uint64_t ctot = scan_counts(
        s_scan, a.tblocks, [&a](uint64_t i) { return a.tsum[i]; }, [&a](uint64_t i, uint64_t at) { a.tsum[i] = at; });
    if (threadIdx.x != 0)
        return;
    const uint64_t bad = a.n ? a.sc[SC_BAD] : U64_MAX;
    /* records and a table of no entries: the missing last entry is entry 0 */
    const uint64_t badtx = a.ntx ? a.sc[SC_BADTX] : (a.n ? 0 : U64_MAX);
    const zslog::Totals t = zslog::totals(a.at, a.start[a.n], ctot, a.ntx, a.finalise != 0);
    const bool inval = bad != U64_MAX || badtx != U64_MAX;
    const uint64_t code = inval ? (uint64_t)(int64_t)ZSCRC_EINVAL : t.end > a.out_cap ? (uint64_t)ZSCRC_ZS_OVERFLOW : 0;
    a.res[0] = code;
    a.res[1] = inval ? bad : a.n;
    a.res[2] = inval ? badtx : t.end;
    a.res[3] = inval ? 0 : t.written;
    a.res[4] = inval ? 0 : t.commits;
    a.res[5] = code ? 0 : t.long_commits;
    a.res[6] = 0;
    a.res[7] = 0;
    a.sc[SC_CODE] = code;
    a.sc[SC_BODY_END] = t.body_end;
    a.tsum[a.tblocks] = ctot;
    /* the finalise commit's span: no bytes, at the commit itself */
    a.sp_off[a.ntx] = code ? 0 : t.body_end;
    a.sp_len[a.ntx] = 0;
    if (!code && a.finalise && a.span_off) {
        a.span_off[a.ntx] = t.body_end;
        a.span_len[a.ntx] = 0;
    }
}

__global__ __launch_bounds__(WG) void log_place_kernel(Log a)
{
    __shared__ uint64_t s_scan[WG / 64];
    const uint64_t first = (uint64_t)blockIdx.x * BLOCK_RECS;
    if (a.sc[SC_CODE] != 0) {
        /* the descriptors empty: the batch reads nothing (some were never written) */
        for (uint32_t k = 0; k < PER; ++k) {
            const uint64_t t = first + k * WG + threadIdx.x;
            if (t < a.ntx)
                a.sp_off[t] = a.sp_len[t] = 0;
        }
        return;
    }
    const uint64_t base = zslog::base_of(a.at);
    uint64_t carry = a.tsum[blockIdx.x];
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k) {
        const uint64_t t = first + k * WG + threadIdx.x;
        const uint64_t len = t < a.ntx ? a.sp_len[t] : 0;
        uint64_t total;
        const uint64_t c = carry + wg_scan(s_scan, t < a.ntx ? commit_len(len) : 0, total);
        if (t < a.ntx) {
            const uint64_t off = zslog::placed(base, a.sp_off[t], c);
            a.cpre[t] = c;
            a.sp_off[t] = off;
            if (a.span_off) {
                a.span_off[t] = off;
                a.span_len[t] = len;
            }
        }
        carry += total;
    }
}

__global__ __launch_bounds__(WG) void log_starts_kernel(Log a)
{
    if (a.sc[SC_CODE] != 0)
        return;
    const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
    if (i > a.n)
        return;
    if (i == a.n) {
        a.start[i] = a.sc[SC_BODY_END]; /* behind every record: the sentinel of the copy */
        return;
    }
    const uint64_t st = zslog::placed(zslog::base_of(a.at), a.start[i], a.cpre[zslog::tx_of(a.tx_end, a.ntx, i)]);
    a.start[i] = st;
    if (a.new_recs)
        a.new_recs[i] = zslog::listed(a.recs[i], st);
}

/* The records in [base, body end) by zscrc_copy_tiles.h's sweep: the starts
 * are file offsets, and the words of the commit records in between are left
 * to the seal. */
__global__ __launch_bounds__(WG) void log_copy_kernel(Log a)
{
    __shared__ uint64_t s_start[LDS_STARTS];
    if (a.sc[SC_CODE] != 0)
        return;
    /* stop > base: there is a record */
    copy_tiles<0, true>(a.src, a.recs, a.start, a.n, a.out, a.tile, zslog::base_of(a.at), a.sc[SC_BODY_END], s_start);
}

__global__ __launch_bounds__(WG) void log_seal_kernel(Log a, Header h)
{
    if (a.sc[SC_CODE] != 0)
        return;
    const uint64_t nc = a.ntx + a.finalise, c = (uint64_t)blockIdx.x * WG + threadIdx.x;
    uint64_t *out = reinterpret_cast<uint64_t *>(a.out);
    if (c == 0) {
        if (a.at == 0)
            for (int i = 0; i < 5; ++i)
                out[i] = h.w[i];
        if (a.ntx == 0)
            a.res[6] = a.prev_crc; /* no span: the register stays */
    }
    if (c >= nc)
        return;
    /* the finalise commit: no bytes, hashed from the register the last span left */
    const uint32_t span_crc = c < a.ntx ? a.crc[c] : a.ntx ? a.crc[a.ntx - 1] : a.prev_crc;
    const uint64_t len = a.sp_len[c], off = a.sp_off[c] + len;
    uint64_t w[3];
    uint32_t stored;
    const int k = commit_words(span_crc, len, false, w, &stored);
    for (int i = 0; i < k; ++i)
        out[off / 8 + i] = w[i];
    if (c + 1 == a.ntx)
        a.res[6] = span_crc;
    if (c + 1 == nc)
        a.res[7] = stored;
}

/* The tile of a call; 0 = a bad option. */
uint64_t tile_of(const zscrc_log_opts *o) { return pow2_opt(o ? o->tile_bytes : 0, DEF_TILE, TILE_MIN, TILE_MAX); }

/* The pieces of the scratch into a, the 8-byte arrays first; the bytes. */
size_t carve(Log &a, zs::Carve c)
{
    a.nblocks = blocks_of(a.n);
    a.tblocks = blocks_of(a.ntx);
    a.sc = c.take<uint64_t>(SC_WORDS, 16);
    a.bsum = c.take<uint64_t>(a.nblocks + 1);
    a.bdel = c.take<uint64_t>(a.nblocks + 1);
    a.start = c.take<uint64_t>(a.n + 1);
    a.tsum = c.take<uint64_t>(a.tblocks + 1);
    a.cpre = c.take<uint64_t>(a.ntx);
    a.sp_off = c.take<uint64_t>(a.ntx + 1);
    a.sp_len = c.take<uint64_t>(a.ntx + 1);
    a.dmark = c.take<uint32_t>(a.n);
    a.crc = c.take<uint32_t>(a.ntx + 1);
    return up16(c.bytes());
}

int launch(Log &a, void *scratch, const Header &h, hipStream_t s)
{
    carve(a, zs::Carve(scratch));
    if (hipMemsetAsync(a.sc + SC_BAD, 0xFF, 16, s) != hipSuccess)
        return ZSCRC_EHIP;
    if (a.n)
        hipLaunchKernelGGL(log_size_kernel, dim3((unsigned)a.nblocks), dim3(WG), 0, s, a);
    hipLaunchKernelGGL(log_scan_kernel, dim3(1), dim3(WG), 0, s, a);
    if (a.n)
        hipLaunchKernelGGL(log_prefix_kernel, dim3((unsigned)a.nblocks), dim3(WG), 0, s, a);
    if (a.ntx)
        hipLaunchKernelGGL(log_tx_kernel, dim3((unsigned)a.tblocks), dim3(WG), 0, s, a);
    hipLaunchKernelGGL(log_txscan_kernel, dim3(1), dim3(WG), 0, s, a);
    if (hipGetLastError() != hipSuccess)
        return ZSCRC_EHIP;
    /* the sizing call ends here */
    if (a.out_cap == 0)
        return ZSCRC_OK;
    if (a.ntx)
        hipLaunchKernelGGL(log_place_kernel, dim3((unsigned)a.tblocks), dim3(WG), 0, s, a);
    if (a.n) {
        /* the bytes written are on the device only: a workgroup a tile that
         * [base, out_cap) can touch */
        const uint64_t base = zslog::base_of(a.at);
        unsigned g;
        if (copy_grid((a.out_cap > base ? a.out_cap - base : 0) + 2 * a.tile, a.tile, COPY_WG_PER_CU, &g) != ZSCRC_OK)
            return ZSCRC_EHIP;
        hipLaunchKernelGGL(log_starts_kernel, dim3((unsigned)(a.n / WG + 1)), dim3(WG), 0, s, a);
        hipLaunchKernelGGL(log_copy_kernel, dim3(g), dim3(WG), 0, s, a);
    }
    if (hipGetLastError() != hipSuccess)
        return ZSCRC_EHIP;
    const uint64_t nc = a.ntx + a.finalise;
    if (nc) {
        const int rc = zscrc_device_batch(a.out, a.sp_off, a.sp_len, nullptr, a.crc, nc, 0, s);
        if (rc)
            return rc;
    }
    hipLaunchKernelGGL(log_seal_kernel, dim3((unsigned)((nc + WG - 1) / WG + (nc ? 0 : 1))), dim3(WG), 0, s, a, h);
    return hipGetLastError() == hipSuccess ? ZSCRC_OK : ZSCRC_EHIP;
}

} /* namespace */

extern "C" {

uint64_t zscrc_device_log_bound(uint64_t n, uint64_t n_commits, uint64_t sum_key_len, uint64_t sum_val_len)
{
    return zslog::bound(n, n_commits, sum_key_len, sum_val_len);
}

size_t zscrc_device_log_scratch_bytes(size_t n, size_t n_tx, const zscrc_log_opts *opts)
{
    if (!tile_of(opts) || n > N_MAX || n_tx > N_MAX)
        return 0;
    Log a{};
    a.n = n;
    a.ntx = n_tx;
    return carve(a, zs::Carve(nullptr));
}

int zscrc_device_log(const void *d_src, uint64_t src_size, const struct zscrc_zs_record *d_recs, size_t n,
                     const uint64_t *d_tx_end, size_t n_tx, const uint8_t uuid[16], uint32_t startidx,
                     uint32_t endidx, void *d_out, uint64_t out_cap, uint64_t at, struct zscrc_zs_record *d_new_recs,
                     uint64_t *d_span_off, uint64_t *d_span_len, uint64_t *d_res, void *scratch,
                     const zscrc_log_opts *opts, unsigned flags, void *stream)
{
    const uint64_t tile = tile_of(opts);
    const uintptr_t oo = reinterpret_cast<uintptr_t>(d_out);
    if (!d_res || (at == 0 && !uuid) || (n && !d_recs) || (n_tx && !d_tx_end) || (!d_span_off != !d_span_len) ||
        (reinterpret_cast<uintptr_t>(scratch) & 15) || (flags & ~ZSCRC_LOG_FINALISE) || !tile ||
        !zslog::counts_ok(n, n_tx, src_size) || !zslog::at_ok(at) || (out_cap && at > out_cap) || (oo & 15) ||
        (!d_out && out_cap) || out_cap > UINTPTR_MAX - oo)
        return ZSCRC_EINVAL;
    /* only the bytes the call may write must not overlap the source */
    const uint64_t room = out_cap ? out_cap - at : 0;
    if (!src_out_ok(d_src, src_size, room ? static_cast<uint8_t *>(d_out) + at : nullptr, room, false))
        return ZSCRC_EINVAL;
    Log a{};
    a.src = static_cast<const uint8_t *>(d_src);
    a.src_size = src_size;
    a.recs = d_recs;
    a.n = n;
    a.tx_end = d_tx_end;
    a.ntx = d_tx_end ? n_tx : n;
    a.out = static_cast<uint8_t *>(d_out);
    a.out_cap = out_cap;
    a.at = at;
    a.new_recs = d_new_recs;
    a.span_off = d_span_off;
    a.span_len = d_span_len;
    a.res = d_res;
    a.tile = tile;
    a.prev_crc = opts ? opts->prev_crc : 0;
    a.finalise = flags & ZSCRC_LOG_FINALISE ? 1 : 0;
    const Header h = at == 0 ? header_words(uuid, startidx, endidx) : Header{};
    hipStream_t s = static_cast<hipStream_t>(stream);
    return zs::with_scratch(scratch, carve(a, zs::Carve(nullptr)), false, s,
                            [&](void *p, zs::Scratch *) { return launch(a, p, h, s); });
}

} /* extern "C" */
