/*
 * zscrc_walk.hip -- the record walk of zscrc_zs_walk (zscrc_zs.cpp) on the
 * device: zscrc_device_walk lists the commit spans of a device-resident
 * active or finalised image without the image ever reaching the host
 * (DESIGN.md 2.6).
 *
 * The walk is a chain off -> step(off), and step(off) depends only on the
 * bytes of the record at off, with step(off) > off.  So the image is cut into
 * blocks (the chain's granularity) of 8-byte slots, and three launches in
 * stream order replace the serial loop:
 *
 *   walk_table_kernel  one workgroup per block: for EVERY slot k of the block
 *                      (whether a record starts there or not) where a walk
 *                      that enters the block at k leaves it (J[k]) and how
 *                      many commits it passes on the way (C[k]); tiles of the
 *                      block last to first, pointer doubling in LDS per tile,
 *                      composed with the finished later tiles
 *   walk_chain_kernel  one lane hops k = J[k] from slot 5 (offset 40), one
 *                      hop per block entered, and records each entered
 *                      block's entry slot and running commit count; it writes
 *                      the result words, and continues with the plain serial
 *                      loop if the chain reaches an unaligned offset
 *   walk_emit_kernel   one workgroup per entered block: marks the slots the
 *                      walk visits from the block's entry (doubling again,
 *                      tiles first to last), prefix-sums the commits among
 *                      them and stores span i at index base + rank
 *
 * No workgroup waits for another one: every phase reads only what an earlier
 * launch (or, inside walk_table_kernel, the same workgroup) wrote.  Every loop
 * is bounded before it starts (doubling rounds = log2 of the tile's slots, at
 * most one hop per block, at most one step per slot in the serial loop).
 * Output positions come from prefix sums: ascending by offset, deterministic.
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>

#include "../../include/zscrc.h"

namespace {

constexpr int WG = 256;
constexpr uint32_t TILE_SLOTS_MAX = 2048;             /* 16 KiB of image per tile */
constexpr uint32_t SPT = TILE_SLOTS_MAX / WG;         /* a thread's slots of a tile: i = thread + j * WG */
constexpr uint64_t DEF_BLOCK = 1ull << 20, DEF_TILE = 16384;
constexpr uint64_t BLOCK_MAX = 1ull << 30;
constexpr uint64_t BLOCKS_MAX = (1ull << 24) - 1;     /* blocks of one image */
constexpr uint32_t J_EXIT = 0x80000000u;              /* J: low bits = the exit record's slot in the block */
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint64_t U64_MAX = ~0ull;
constexpr uint64_t HDR = 40;

enum {
    T_KEY = 1, T_VALUE = 2, T_COMMIT = 4, T_FINAL = 16, T_DELETED = 64,
    T_LONG_KEY = 33, T_LONG_COMMIT = 36, T_LONG_FINAL = 48, T_LONG_DELETED_ALIAS = 32,
};
enum { S_ADV = 0, S_COMMIT = 1, S_TRUNC = 2, S_STOP = 3 };

struct Step {
    uint32_t kind;  /* S_ADV / S_COMMIT: the walk goes on at next */
    uint64_t next;
    uint64_t span;  /* S_COMMIT: the span is [off - span, off) */
};

/* An entered block: the slot (in the block) the walk enters it at and the
 * commits before it; slot NONE = the walk skips the block. */
struct Entry {
    uint32_t slot;
    uint32_t pad;
    uint64_t base;
};

struct Walk {
    const uint8_t *img;
    uint64_t size;
    uint64_t ns;          /* slots: ceil(size / 8) (a last partial slot is TRUNCATED) */
    uint32_t bs, ts;      /* slots per block, per tile (powers of two, ts <= bs) */
    uint32_t rounds;      /* log2(ts) */
    uint64_t nblocks;
    Entry *entry;         /* scratch: nblocks */
    uint32_t *J, *C;      /* scratch: ns each */
    uint64_t *off, *len;
    uint64_t cap;
    uint64_t *res;
};

/* Big-endian 64-bit word at any byte address. */
__device__ __forceinline__ uint64_t be64(const uint8_t *p)
{
    if ((reinterpret_cast<uintptr_t>(p) & 7) == 0)
        return __builtin_bswap64(*reinterpret_cast<const uint64_t *>(p));
    uint64_t v = 0;
    for (int i = 0; i < 8; ++i)
        v = (v << 8) | p[i];
    return v;
}

__device__ __forceinline__ uint64_t rup8(uint64_t n) { return (n + 7) & ~7ull; }

/* The record word at off < size, 0 where fewer than 8 bytes are left. */
__device__ __forceinline__ uint64_t word_at(const uint8_t *img, uint64_t size, uint64_t off)
{
    return size - off >= 8 ? be64(img + off) : 0;
}

/* One iteration of zscrc_zs_walk's loop at off < size (commit_at included):
 * the same room checks (never an add that can wrap), the same classes.
 * Reads nothing outside [img, img + size); next > off and next <= size.
 * w = word_at(off): the tile sweeps load their slots' words ahead of the
 * steps, so that the loads of a thread's slots are in flight together. */
__device__ Step step_w(const uint8_t *img, uint64_t size, uint64_t off, uint64_t w)
{
    Step s{S_TRUNC, off, 0};
    const uint64_t room = size - off;
    if (room < 8)
        return s;
    const unsigned t = (unsigned)(w >> 56);
    if (t == T_KEY || t == T_LONG_KEY) {
        uint64_t voff;
        if (t == T_KEY) {
            voff = w & 0xFFFFFFFFull;
        } else {
            if (room < 24)
                return s;
            voff = be64(img + off + 16);
        }
        if (voff == 0 || voff > room || room - voff < 16)
            return s;
        const uint64_t v = off + voff;
        const uint64_t vw = be64(img + v);
        const uint64_t vlen = (vw >> 56) == T_VALUE ? ((vw >> 32) & 0xFFFFFF) : be64(img + v + 8);
        const uint64_t vroom = size - v - 16;
        if (vlen > vroom || rup8(vlen) > vroom)
            return s;
        s.kind = S_ADV;
        s.next = v + 16 + rup8(vlen);
    } else if (t == T_DELETED || t == T_LONG_DELETED_ALIAS) {
        if (room < 24)
            return s;
        const uint64_t klen = t == T_DELETED ? ((w >> 40) & 0xFFFF) : be64(img + off + 8);
        if (klen > room - 24 || rup8(klen) > room - 24)
            return s;
        s.kind = S_ADV;
        s.next = off + 24 + rup8(klen);
    } else if (t == T_COMMIT) {
        const uint64_t sl = (w >> 32) & 0xFFFFFF;
        if (sl > off)
            return s;
        s.kind = S_COMMIT;
        s.span = sl;
        s.next = off + 8;
    } else if (t == T_LONG_COMMIT) {
        if (room < 24)
            return s;
        const uint64_t sl = be64(img + off + 8);
        if (sl > off)
            return s;
        s.kind = S_COMMIT;
        s.span = sl;
        s.next = off + 24;
    } else {
        s.kind = S_STOP;
    }
    return s;
}

__device__ __forceinline__ Step step(const uint8_t *img, uint64_t size, uint64_t off)
{
    return step_w(img, size, off, word_at(img, size, off));
}

/* Where the walk goes from slot k (first slot of its block: b0, the block ends
 * before slot bend): the next slot when that is a slot of the same block
 * (the link the doubling follows), else NONE -- the record at k is then the
 * chain's last one in the block (its exit record). */
__device__ __forceinline__ uint64_t link_of(const Step &s, uint64_t bend)
{
    if (s.kind > S_COMMIT || (s.next & 7))
        return U64_MAX;
    const uint64_t n = s.next >> 3;
    return n < bend ? n : U64_MAX;
}

/* J of an exit record at slot k of the block starting at b0. */
__device__ __forceinline__ uint32_t exit_code(const Step &s, uint64_t k, uint64_t b0)
{
    if (s.kind <= S_COMMIT && !(s.next & 7)) {
        const uint64_t rel = (s.next >> 3) - b0;
        if (rel < J_EXIT)
            return (uint32_t)rel;
    }
    /* a stop, an unaligned next or a jump of 16 GiB and more: the chain
     * kernel evaluates the record itself */
    return J_EXIT | (uint32_t)(k - b0);
}

__global__ __launch_bounds__(WG) void walk_table_kernel(Walk a)
{
    __shared__ uint32_t s_p[TILE_SLOTS_MAX];   /* link (slot in the tile); a root points at itself */
    __shared__ uint32_t s_acc[TILE_SLOTS_MAX]; /* commits from the slot up to its link, exclusive */
    __shared__ uint32_t s_rj[TILE_SLOTS_MAX];  /* roots: J and C of the root itself */
    __shared__ uint32_t s_rc[TILE_SLOTS_MAX];
    const uint64_t b0 = (uint64_t)blockIdx.x * a.bs;
    const uint64_t bend = b0 + a.bs < a.ns ? b0 + a.bs : a.ns;
    const uint32_t tiles = (uint32_t)((bend - b0 + a.ts - 1) / a.ts);
    for (uint32_t t = tiles; t-- > 0;) {
        const uint64_t t0 = b0 + (uint64_t)t * a.ts;
        uint64_t w[SPT];
#pragma unroll
        for (uint32_t j = 0; j < SPT; ++j) {
            const uint64_t k = t0 + threadIdx.x + j * WG;
            w[j] = threadIdx.x + j * WG < a.ts && k < bend ? word_at(a.img, a.size, k << 3) : 0;
        }
#pragma unroll
        for (uint32_t j = 0; j < SPT; ++j) {
            const uint32_t i = threadIdx.x + j * WG;
            if (i >= a.ts)
                break;
            const uint64_t k = t0 + i;
            uint32_t p = i, acc = 0, rj = 0, rc = 0;
            if (k < bend) {
                const Step s = step_w(a.img, a.size, k << 3, w[j]);
                const uint32_t cm = s.kind == S_COMMIT;
                const uint64_t n = link_of(s, bend);
                if (n == U64_MAX) {
                    rj = exit_code(s, k, b0);
                    rc = cm;
                } else if (n - t0 < a.ts) {
                    p = (uint32_t)(n - t0);
                    acc = cm;
                } else { /* a later tile of this block, finished by this workgroup */
                    rj = a.J[n];
                    rc = a.C[n] + cm;
                }
            }
            s_p[i] = p;
            s_acc[i] = acc;
            s_rj[i] = rj;
            s_rc[i] = rc;
        }
        __syncthreads();
        for (uint32_t r = 0; r < a.rounds; ++r) {
            /* ts <= 8 * WG: a thread's slots of one round in registers */
            uint32_t np[SPT], na[SPT];
            int moved = 0;
#pragma unroll
            for (uint32_t j = 0; j < SPT; ++j) {
                const uint32_t i = threadIdx.x + j * WG;
                if (i < a.ts) {
                    const uint32_t p = s_p[i];
                    np[j] = s_p[p];
                    na[j] = s_acc[i] + s_acc[p];
                    moved |= np[j] != p;
                }
            }
            /* no link moved: every slot points at its root already (short
             * chains need fewer rounds than the bound) */
            if (!__syncthreads_or(moved))
                break;
#pragma unroll
            for (uint32_t j = 0; j < SPT; ++j) {
                const uint32_t i = threadIdx.x + j * WG;
                if (i < a.ts) {
                    s_p[i] = np[j];
                    s_acc[i] = na[j];
                }
            }
            __syncthreads();
        }
        for (uint32_t i = threadIdx.x; i < a.ts; i += WG) {
            const uint64_t k = t0 + i;
            if (k < bend) {
                const uint32_t root = s_p[i];
                a.J[k] = s_rj[root];
                a.C[k] = s_acc[i] + s_rc[root];
            }
        }
        /* the next (earlier) tile reads this one's J and C from memory: the
         * barrier orders this workgroup's stores before its own loads */
        __threadfence_block();
        __syncthreads();
    }
}

/* The plain loop of zscrc_zs_walk from (off, n), one lane; at most one step
 * per slot.  Spans go to index n onwards; mn / mx fold their lengths. */
__device__ void serial_walk(const Walk &a, uint64_t off, uint64_t n, uint64_t mx, uint64_t mn, uint64_t took_over)
{
    int rc = ZSCRC_ZS_END;
    for (uint64_t it = 0; it <= a.ns && off < a.size; ++it) {
        const Step s = step(a.img, a.size, off);
        if (s.kind == S_TRUNC) {
            rc = ZSCRC_ZS_TRUNCATED;
            break;
        }
        if (s.kind == S_STOP) {
            rc = ZSCRC_ZS_STOPPED;
            break;
        }
        if (s.kind == S_COMMIT) {
            if (n < a.cap) {
                a.off[n] = off - s.span;
                a.len[n] = s.span;
            }
            mx = s.span > mx ? s.span : mx;
            mn = s.span < mn ? s.span : mn;
            ++n;
        }
        off = s.next;
    }
    a.res[0] = n > a.cap ? (uint64_t)ZSCRC_ZS_OVERFLOW : (uint64_t)rc;
    a.res[1] = n;
    a.res[2] = off;
    a.res[3] = mx;
    /* the emit launch folds the blocks' lengths into [3] and [4] */
    a.res[4] = n ? mn : 0;
    a.res[5] = took_over;
}

__global__ __launch_bounds__(64) void walk_serial_kernel(Walk a)
{
    if (threadIdx.x == 0 && blockIdx.x == 0)
        serial_walk(a, HDR, 0, 0, U64_MAX, U64_MAX);
}

__global__ __launch_bounds__(WG) void walk_chain_kernel(Walk a)
{
    for (uint64_t b = threadIdx.x; b < a.nblocks; b += WG)
        a.entry[b].slot = NONE;
    __syncthreads();
    if (threadIdx.x != 0)
        return;
    uint64_t k = HDR / 8, n = 0, end = 0;
    int rc = -1; /* -1: the chain goes on */
    uint64_t unaligned = U64_MAX;
    for (uint64_t hop = 0; hop <= a.nblocks; ++hop) {
        if (k >= a.ns) { /* a next offset is <= size: this is off == size */
            rc = ZSCRC_ZS_END;
            end = a.size;
            break;
        }
        const uint64_t b = k / a.bs, b0 = b * a.bs;
        a.entry[b].slot = (uint32_t)(k - b0);
        a.entry[b].base = n;
        const uint32_t j = a.J[k];
        n += a.C[k];
        if (!(j & J_EXIT)) {
            k = b0 + j;
            continue;
        }
        const uint64_t e = (b0 + (j & ~J_EXIT)) << 3;
        const Step s = step(a.img, a.size, e);
        if (s.kind == S_TRUNC || s.kind == S_STOP) {
            rc = s.kind == S_TRUNC ? ZSCRC_ZS_TRUNCATED : ZSCRC_ZS_STOPPED;
            end = e;
            break;
        }
        if (s.next & 7) {
            unaligned = s.next;
            break;
        }
        k = s.next >> 3;
    }
    if (unaligned != U64_MAX) {
        serial_walk(a, unaligned, n, 0, U64_MAX, unaligned);
        return;
    }
    a.res[0] = n > a.cap ? (uint64_t)ZSCRC_ZS_OVERFLOW : (uint64_t)rc;
    a.res[1] = n;
    a.res[2] = end;
    a.res[3] = 0;
    a.res[4] = n ? U64_MAX : 0;
    a.res[5] = U64_MAX;
}

__global__ __launch_bounds__(WG) void walk_emit_kernel(Walk a)
{
    __shared__ uint32_t s_p[TILE_SLOTS_MAX]; /* link; after the doubling: 1 = a visited commit */
    __shared__ uint32_t s_m[TILE_SLOTS_MAX]; /* 1 = the walk visits the slot */
    __shared__ uint32_t s_scan[2][WG];
    __shared__ uint32_t s_cur;               /* the walk's next slot in the block, NONE = it left */
    __shared__ unsigned long long s_mx, s_mn;
    const Entry en = a.entry[blockIdx.x];
    if (en.slot == NONE)
        return;
    const uint64_t b0 = (uint64_t)blockIdx.x * a.bs;
    const uint64_t bend = b0 + a.bs < a.ns ? b0 + a.bs : a.ns;
    const uint32_t tiles = (uint32_t)((bend - b0 + a.ts - 1) / a.ts);
    const uint32_t per = a.ts > WG ? a.ts / WG : 1; /* slots per thread of the scan, contiguous */
    uint64_t base = en.base, mx = 0, mn = U64_MAX;
    if (threadIdx.x == 0) {
        s_cur = en.slot;
        s_mx = 0;
        s_mn = U64_MAX;
    }
    __syncthreads();
    for (uint32_t t = 0; t < tiles; ++t) {
        const uint32_t cur = s_cur;
        if (cur == NONE)
            break;
        if (cur / a.ts != t) /* a record longer than the tile: the walk skips it */
            continue;
        const uint64_t t0 = b0 + (uint64_t)t * a.ts;
        const uint64_t tend = t0 + a.ts < bend ? t0 + a.ts : bend;
        __syncthreads(); /* every thread has read s_cur */
        uint64_t w[SPT];
#pragma unroll
        for (uint32_t j = 0; j < SPT; ++j) {
            const uint64_t k = t0 + threadIdx.x + j * WG;
            w[j] = threadIdx.x + j * WG < a.ts && k < bend ? word_at(a.img, a.size, k << 3) : 0;
        }
#pragma unroll
        for (uint32_t j = 0; j < SPT; ++j) {
            const uint32_t i = threadIdx.x + j * WG;
            if (i >= a.ts)
                break;
            const uint64_t k = t0 + i;
            uint32_t p = i;
            if (k < bend) {
                const uint64_t n = link_of(step_w(a.img, a.size, k << 3, w[j]), tend);
                if (n != U64_MAX)
                    p = (uint32_t)(n - t0);
            }
            s_p[i] = p;
            s_m[i] = i == cur - t * a.ts;
        }
        if (threadIdx.x == 0)
            s_cur = NONE;
        __syncthreads();
        /* after round r the slots up to 2^(r+1) - 1 links from the entry are
         * marked; a mark seen early only marks a later slot of the same chain */
        for (uint32_t r = 0; r < a.rounds; ++r) {
            uint32_t np[SPT];
            int moved = 0;
#pragma unroll
            for (uint32_t j = 0; j < SPT; ++j) {
                const uint32_t i = threadIdx.x + j * WG;
                if (i < a.ts) {
                    const uint32_t p = s_p[i];
                    if (s_m[i])
                        s_m[p] = 1;
                    np[j] = s_p[p];
                    moved |= np[j] != p;
                }
            }
            /* no link moved: the links reached their roots a round ago, so
             * this round's marks were the last ones */
            if (!__syncthreads_or(moved))
                break;
#pragma unroll
            for (uint32_t j = 0; j < SPT; ++j) {
                const uint32_t i = threadIdx.x + j * WG;
                if (i < a.ts)
                    s_p[i] = np[j];
            }
            __syncthreads();
        }
        /* visited slots: the commits among them, and where the walk goes
         * from the last one (the one visited slot without a link) */
        for (uint32_t i = threadIdx.x; i < a.ts; i += WG) {
            uint32_t f = 0;
            if (s_m[i]) {
                const Step s = step(a.img, a.size, (t0 + i) << 3);
                f = s.kind == S_COMMIT;
                if (link_of(s, tend) == U64_MAX) {
                    const uint64_t n = link_of(s, bend);
                    s_cur = n == U64_MAX ? NONE : (uint32_t)(n - b0);
                }
            }
            s_p[i] = f;
        }
        __syncthreads();
        /* rank of each visited commit: prefix sum in slot order */
        uint32_t mine = 0;
        const uint32_t first = threadIdx.x * per;
        if (first < a.ts)
            for (uint32_t j = 0; j < per; ++j)
                mine += s_p[first + j];
        int cur_buf = 0;
        s_scan[0][threadIdx.x] = mine;
        __syncthreads();
        for (uint32_t d = 1; d < WG; d <<= 1) {
            uint32_t v = s_scan[cur_buf][threadIdx.x];
            if (threadIdx.x >= d)
                v += s_scan[cur_buf][threadIdx.x - d];
            s_scan[cur_buf ^ 1][threadIdx.x] = v;
            cur_buf ^= 1;
            __syncthreads();
        }
        const uint32_t total = s_scan[cur_buf][WG - 1];
        uint64_t rank = base + s_scan[cur_buf][threadIdx.x] - mine;
        if (mine) {
            for (uint32_t j = 0; j < per; ++j) {
                if (!s_p[first + j])
                    continue;
                const uint64_t off = (t0 + first + j) << 3;
                const Step s = step(a.img, a.size, off);
                if (rank < a.cap) {
                    a.off[rank] = off - s.span;
                    a.len[rank] = s.span;
                }
                mx = s.span > mx ? s.span : mx;
                mn = s.span < mn ? s.span : mn;
                ++rank;
            }
        }
        base += total;
        __syncthreads(); /* s_p, s_scan and s_cur are rewritten by the next tile */
    }
    if (mn != U64_MAX) {
        atomicMax(&s_mx, (unsigned long long)mx);
        atomicMin(&s_mn, (unsigned long long)mn);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_mn != U64_MAX) {
        atomicMax(reinterpret_cast<unsigned long long *>(a.res + 3), s_mx);
        atomicMin(reinterpret_cast<unsigned long long *>(a.res + 4), s_mn);
    }
}

/* ------------------------------------------------------------------ host */

bool pow2(uint64_t v) { return v && !(v & (v - 1)); }

/* The geometry for an image: false = bad options. */
bool geometry(uint64_t size, const zscrc_walk_opts *o, Walk *w)
{
    const uint64_t block = o && o->block_bytes ? o->block_bytes : DEF_BLOCK;
    uint64_t tile = o && o->tile_bytes ? o->tile_bytes : DEF_TILE;
    if (!(o && o->tile_bytes) && tile > block)
        tile = block;
    if (!pow2(block) || block < 64 || block > BLOCK_MAX || !pow2(tile) || tile < 64 || tile > block ||
        tile > 8ull * TILE_SLOTS_MAX)
        return false;
    w->size = size;
    w->ns = size / 8 + (size % 8 != 0);
    w->bs = (uint32_t)(block / 8);
    w->ts = (uint32_t)(tile / 8);
    w->rounds = (uint32_t)__builtin_ctz(w->ts);
    w->nblocks = (w->ns + w->bs - 1) / w->bs;
    /* one workgroup per block: a grid's threads must stay below 2^32 */
    return w->nblocks <= BLOCKS_MAX;
}

/* The one-lane walk alone: asked for, or an image of less than one tile. */
bool serial_only(const Walk &w, unsigned flags) { return (flags & ZSCRC_WALK_SERIAL) || w.ns < w.ts; }

size_t scratch_bytes(const Walk &w) { return (size_t)(w.nblocks * sizeof(Entry) + w.ns * 8); }

/* Library-owned scratch, one buffer per device, shared by every call there: a
 * call on another stream than the last user's waits for that user's work. */
constexpr int MAX_DEV = 64;
struct Scratch {
    std::mutex mu;
    void *p = nullptr;
    size_t bytes = 0;
    hipEvent_t last = nullptr;
    hipStream_t last_stream = nullptr;
    bool last_valid = false;
};
Scratch g_scratch[MAX_DEV];

/* Whether the handles certainly name one stream: hipStreamPerThread is a
 * different stream in every host thread (never equal, a wait on a stream's
 * own event being harmless), hipStreamLegacy is the NULL stream. */
bool same_stream(hipStream_t a, hipStream_t b)
{
    if (a == hipStreamLegacy)
        a = nullptr;
    if (b == hipStreamLegacy)
        b = nullptr;
    return a == b && a != hipStreamPerThread;
}

int launch(const Walk &w, unsigned flags, hipStream_t s)
{
    if (serial_only(w, flags)) {
        hipLaunchKernelGGL(walk_serial_kernel, dim3(1), dim3(64), 0, s, w);
    } else {
        hipLaunchKernelGGL(walk_table_kernel, dim3((unsigned)w.nblocks), dim3(WG), 0, s, w);
        hipLaunchKernelGGL(walk_chain_kernel, dim3(1), dim3(WG), 0, s, w);
        hipLaunchKernelGGL(walk_emit_kernel, dim3((unsigned)w.nblocks), dim3(WG), 0, s, w);
    }
    return hipGetLastError() == hipSuccess ? ZSCRC_OK : ZSCRC_EHIP;
}

} /* namespace */

extern "C" {

size_t zscrc_device_walk_scratch_bytes(uint64_t image_size, const zscrc_walk_opts *opts)
{
    Walk w{};
    if (!geometry(image_size, opts, &w))
        return 0;
    return scratch_bytes(w);
}

int zscrc_device_walk(const void *d_image, uint64_t image_size, uint64_t *d_span_off, uint64_t *d_span_len,
                      size_t cap, uint64_t *d_res, void *scratch, const zscrc_walk_opts *opts, unsigned flags,
                      void *stream)
{
    Walk w{};
    if (!d_image || image_size < HDR || !d_res || (cap && (!d_span_off || !d_span_len)) ||
        (flags & ~ZSCRC_WALK_SERIAL) || !geometry(image_size, opts, &w) ||
        (reinterpret_cast<uintptr_t>(scratch) & 15))
        return ZSCRC_EINVAL;
    w.img = static_cast<const uint8_t *>(d_image);
    w.off = d_span_off;
    w.len = d_span_len;
    w.cap = cap;
    w.res = d_res;
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto place = [&w](void *p) {
        w.entry = static_cast<Entry *>(p);
        w.J = reinterpret_cast<uint32_t *>(w.entry + w.nblocks);
        w.C = w.J + w.ns;
    };
    if (serial_only(w, flags)) /* touches no scratch */
        return launch(w, flags, s);
    if (scratch) {
        place(scratch);
        return launch(w, flags, s);
    }
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEV)
        return ZSCRC_ENODEV;
    Scratch &sc = g_scratch[dev];
    std::lock_guard<std::mutex> lk(sc.mu);
    const size_t need = scratch_bytes(w);
    if (sc.bytes < need) {
        if (sc.p)
            (void)hipFree(sc.p); /* waits for the device: no user is left */
        sc.p = nullptr;
        sc.bytes = 0;
        sc.last_valid = false;
        /* about the image's size: no slack on top */
        if (hipMalloc(&sc.p, need) != hipSuccess) {
            sc.p = nullptr;
            return ZSCRC_ENOMEM;
        }
        sc.bytes = need;
    }
    if (sc.last_valid && !same_stream(sc.last_stream, s) && hipStreamWaitEvent(s, sc.last, 0) != hipSuccess)
        return ZSCRC_EHIP;
    place(sc.p);
    const int rc = launch(w, flags, s);
    if (!sc.last && hipEventCreateWithFlags(&sc.last, hipEventDisableTiming) != hipSuccess)
        sc.last = nullptr;
    sc.last_valid = sc.last && hipEventRecord(sc.last, s) == hipSuccess;
    sc.last_stream = s;
    if (!sc.last_valid && rc == ZSCRC_OK) /* no event to order the next user by: drain instead */
        return hipStreamSynchronize(s) == hipSuccess ? ZSCRC_OK : ZSCRC_EHIP;
    return rc;
}

/* zscrc_release_cache(): the walk's scratch, every device. */
void zs_walk_release_cache(void)
{
    int cur = -1;
    (void)hipGetDevice(&cur);
    for (int d = 0; d < MAX_DEV; ++d) {
        Scratch &sc = g_scratch[d];
        std::lock_guard<std::mutex> lk(sc.mu);
        if (!sc.p && !sc.last)
            continue;
        (void)hipSetDevice(d);
        if (sc.p)
            (void)hipFree(sc.p);
        if (sc.last)
            (void)hipEventDestroy(sc.last);
        sc.p = nullptr;
        sc.bytes = 0;
        sc.last = nullptr;
        sc.last_valid = false;
    }
    if (cur >= 0)
        (void)hipSetDevice(cur);
}

} /* extern "C" */
