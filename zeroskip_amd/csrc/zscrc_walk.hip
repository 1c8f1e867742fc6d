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
 *
 * zscrc_device_walk_multi (further down) is the same walk over many images of
 * one device buffer in four launches, and zscrc_device_verify_images the
 * verification of all of them on top of it.  Its kernels run the single
 * walk's bodies on a Walk view of each image: table_sweep, chain_hops,
 * emit_sweep and serial_loop are written once, and the kernels of both walks
 * keep only what differs around them.
 *
 * The bodies take a step policy: what one iteration of the host loop does at
 * an offset, which records are put out and what is folded over them.
 * CommitWalk (zscrc_zs_walk's loop, the spans) is the policy of every kernel
 * above; RecordList (zscrc_zs_records' loop, shared with the host through
 * zscrc_records.h) makes zscrc_device_records the same three launches with
 * 32-byte record entries as output.  The two host loops differ on corrupt
 * images (the lister never looks at a commit's span length, the walk never at
 * a key length), so neither can use the other's tables.  Packed images have no
 * chain: records_packed_*_kernel parse the pointer section one pointer a thread.
 * zscrc_device_records_multi is RecordList over many images, the fourth
 * combination: the many-image walk's four launches with this policy.
 *
 * Shared with the other device stages: the record words and types
 * (zscrc_records.h), the many-image walk's scan of the counts (scan_counts,
 * zscrc_wg.h; the emit sweep keeps a scan of its own, tile_scan) and the
 * scratch of a call (zs::with_scratch, zscrc_internal.h; the library's buffer
 * and its pinned staging: zscrc_scratch.cpp).
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "../../include/zscrc.h"
#include "zscrc_internal.h"
#include "zscrc_records.h"
#include "zscrc_wg.h"

namespace {

using namespace zsdev;
using namespace zsrec; /* be64, rup8, HDR, U64_MAX and the record types T_* */
using zs::Scratch;

constexpr uint32_t TILE_SLOTS_MAX = 2048;            /* 16 KiB of image per tile */
constexpr uint32_t SPT = TILE_SLOTS_MAX / WG;         /* a thread's slots of a tile: i = thread + j * WG */
constexpr uint64_t DEF_BLOCK = 1ull << 20, DEF_TILE = 16384;
constexpr uint64_t BLOCK_MAX = 1ull << 30;
constexpr uint64_t BLOCKS_MAX = (1ull << 24) - 1;     /* blocks of one image */
constexpr uint32_t J_EXIT = 0x80000000u;              /* J: low bits = the exit record's slot in the block */
constexpr uint32_t NONE = 0xFFFFFFFFu;

/* What a step finds: S_OUT = a record the walk puts out (the commit walk: a
 * commit, S_COMMIT; the record lister: a key or delete record), S_ADV = one it
 * only advances over; the shared bodies look at nothing else of a kind. */
enum { S_ADV = 0, S_OUT = 1, S_COMMIT = S_OUT, S_TRUNC = 2, S_STOP = 3 };

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
    uint64_t *off, *len;  /* the spans (RecordList: off = the record entries, four words each; len unused) */
    uint64_t cap;
    uint64_t *res;
};

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
    } else if (t == T_DELETED || t == T_LONG_DELETED) {
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

/* The step of policy P at off < size, its word loaded here. */
template <class P>
__device__ __forceinline__ typename P::S step(const uint8_t *img, uint64_t size, uint64_t off)
{
    return P::step_w(img, size, off, word_at(img, size, off));
}

/* Where the walk goes from slot k (first slot of its block: b0, the block ends
 * before slot bend): the next slot when that is a slot of the same block
 * (the link the doubling follows), else NONE -- the record at k is then the
 * chain's last one in the block (its exit record). */
template <class S>
__device__ __forceinline__ uint64_t link_of(const S &s, uint64_t bend)
{
    if (s.kind > S_OUT || (s.next & 7))
        return U64_MAX;
    const uint64_t n = s.next >> 3;
    return n < bend ? n : U64_MAX;
}

/* J of an exit record at slot k of the block starting at b0. */
template <class S>
__device__ __forceinline__ uint32_t exit_code(const S &s, uint64_t k, uint64_t b0)
{
    if (s.kind <= S_OUT && !(s.next & 7)) {
        const uint64_t rel = (s.next >> 3) - b0;
        if (rel < J_EXIT)
            return (uint32_t)rel;
    }
    /* a stop, an unaligned next or a jump of 16 GiB and more: the chain
     * kernel evaluates the record itself */
    return J_EXIT | (uint32_t)(k - b0);
}

/* The words of a thread's slots of the tile at slot t0 (0 past the tile or
 * the block's end, bend), loaded ahead of the steps that take them. */
__device__ __forceinline__ void tile_words(const Walk &a, uint64_t t0, uint64_t bend, uint64_t (&w)[SPT])
{
#pragma unroll
    for (uint32_t j = 0; j < SPT; ++j) {
        const uint64_t k = t0 + threadIdx.x + j * WG;
        w[j] = threadIdx.x + j * WG < a.ts && k < bend ? word_at(a.img, a.size, k << 3) : 0;
    }
}

/* The emit sweep's scan: inclusive prefix sum over the workgroup's threads of
 * one value each, double-buffered in LDS; total = the last thread's.  The
 * caller's next barrier comes before s changes.  (Every other scan is
 * zscrc_wg.h's wg_scan; this one stays until a change to the hot emit kernels
 * is measured on its own.) */
template <class T>
__device__ __forceinline__ T tile_scan(T (&s)[2][WG], T mine, T &total)
{
    int cur = 0;
    s[0][threadIdx.x] = mine;
    __syncthreads();
    for (uint32_t d = 1; d < WG; d <<= 1) {
        T v = s[cur][threadIdx.x];
        if (threadIdx.x >= d)
            v += s[cur][threadIdx.x - d];
        s[cur ^ 1][threadIdx.x] = v;
        cur ^= 1;
        __syncthreads();
    }
    total = s[cur][WG - 1];
    return s[cur][threadIdx.x];
}

/* What the many-image walk adds to a span on its way out: the arena offset of
 * the image's first byte, the image's index and the totals' words. */
struct Multi {
    uint64_t add;
    uint32_t *img;   /* d_span_img */
    uint32_t j;
    uint64_t *tot;
};

/* The span [at, at + span) of the image as output entry `rank`, if there is
 * room for it (the many-image walk: its arena offset, its image beside it);
 * mx / mn fold its length either way. */
template <bool MULTI>
__device__ __forceinline__ void put_span(const Walk &a, const Multi &m, uint64_t rank, uint64_t at, uint64_t span,
                                         uint64_t &mx, uint64_t &mn)
{
    if (rank < a.cap) {
        a.off[rank] = MULTI ? m.add + at : at;
        a.len[rank] = span;
        if constexpr (MULTI)
            m.img[rank] = m.j;
    }
    mx = span > mx ? span : mx;
    mn = span < mn ? span : mn;
}

/* Folds a longest and a shortest length into the words w[0] (max), w[1] (min). */
__device__ __forceinline__ void fold_lengths(uint64_t *w, uint64_t mx, uint64_t mn)
{
    atomicMax(reinterpret_cast<unsigned long long *>(w), (unsigned long long)mx);
    atomicMin(reinterpret_cast<unsigned long long *>(w + 1), (unsigned long long)mn);
}

/* A step policy is what the shared bodies (table_sweep, chain_hops,
 * emit_sweep, serial_loop, serial_walk, chain_walk) are instances of:
 *   S          a step's result: kind, next, and what put() needs of the record
 *   step_w     one iteration of the host loop at off < size, w = word_at(off);
 *              reads nothing outside the image, next > off and next <= size
 *   Acc        what a thread folds over the records it puts out
 *   put        the S_OUT record at `at` as output entry `rank` (stored if
 *              rank < cap), folded into acc either way
 *   fold_init / fold_lds / folded / fold_out
 *              a workgroup's Accs folded in FOLD words of LDS, then into the
 *              result words: order-independent integer atomics only
 *   finish     the result words, by the one lane that knows them
 * CommitWalk is zscrc_zs_walk's loop (the commit spans), RecordList
 * zscrc_zs_records' (the key and delete records). */
struct CommitWalk {
    using S = Step;
    struct Acc {
        uint64_t mx = 0, mn = U64_MAX;
    };
    static constexpr int FOLD = 2;
    /* the many-image rows: words a row, the take-over word, the first-index word */
    static constexpr int ROW = ZSCRC_WALK_ROW_WORDS, TAKE = 5, FIRST = 6;
    static constexpr bool TOT_NOT_END = false;
    static __device__ __forceinline__ S step_w(const uint8_t *img, uint64_t size, uint64_t off, uint64_t w)
    {
        return ::step_w(img, size, off, w);
    }
    template <bool MULTI>
    static __device__ __forceinline__ void put(const Walk &a, const Multi &m, uint64_t rank, uint64_t at, const S &s,
                                               Acc &acc)
    {
        put_span<MULTI>(a, m, rank, at - s.span, s.span, acc.mx, acc.mn);
    }
    static __device__ __forceinline__ void fold_init(uint64_t *w)
    {
        w[0] = 0;
        w[1] = U64_MAX;
    }
    static __device__ __forceinline__ void fold_lds(uint64_t *w, const Acc &acc)
    {
        if (acc.mn != U64_MAX)
            fold_lengths(w, acc.mx, acc.mn);
    }
    static __device__ __forceinline__ bool folded(const uint64_t (&w)[FOLD]) { return w[1] != U64_MAX; }
    static __device__ __forceinline__ void acc_words(const Acc &acc, uint64_t (&w)[FOLD])
    {
        w[0] = acc.mx;
        w[1] = acc.mn;
    }
    template <bool MULTI>
    static __device__ __forceinline__ void fold_out(const Walk &a, const Multi &m, uint64_t *w)
    {
        fold_lengths(a.res + 3, w[0], w[1]);
        if constexpr (MULTI)
            fold_lengths(m.tot + 2, w[0], w[1]);
    }
    /* the totals' fold words [2] and [3] for n commits; `bad` is not kept */
    static __device__ __forceinline__ void tot_init(uint64_t *tot, uint64_t n, uint64_t)
    {
        tot[2] = 0;
        tot[3] = n ? U64_MAX : 0;
    }
    /* the emit launch folds the blocks' lengths into [3] and [4] */
    static __device__ __forceinline__ void finish(const Walk &a, int rc, uint64_t n, uint64_t end, const Acc &acc,
                                                  uint64_t took_over)
    {
        a.res[0] = n > a.cap ? (uint64_t)ZSCRC_ZS_OVERFLOW : (uint64_t)rc;
        a.res[1] = n;
        a.res[2] = end;
        a.res[3] = acc.mx;
        a.res[4] = n ? acc.mn : 0;
        a.res[5] = took_over;
    }
};

/* The record lister: Walk::off holds the zscrc_zs_record array (four words an
 * entry), Walk::len nothing; res = ZSCRC_RECORDS_RES_WORDS words. */
struct RStep {
    uint32_t kind;
    uint64_t next;
    zscrc_zs_record rec;
};

struct RecordList {
    using S = RStep;
    struct Acc {
        uint64_t del = 0, klen = 0, vlen = 0, kmax = 0, vmax = 0;
    };
    static constexpr int FOLD = 5;
    static constexpr int ROW = ZSCRC_RECORDS_ROW_WORDS, TAKE = 8, FIRST = 9;
    static constexpr bool TOT_NOT_END = true;
    static_assert(ROW == ZSCRC_RECORDS_RES_WORDS, "finish writes a row");
    /* zsrec::L_SKIP / L_RECORD / L_TRUNC / L_STOP are S_ADV / S_OUT / S_TRUNC / S_STOP */
    static __device__ __forceinline__ S step_w(const uint8_t *img, uint64_t size, uint64_t off, uint64_t w)
    {
        static_assert(zsrec::L_SKIP == S_ADV && zsrec::L_RECORD == S_OUT && zsrec::L_TRUNC == S_TRUNC &&
                          zsrec::L_STOP == S_STOP,
                      "the lister's classes are the walk's");
        S s;
        s.next = off;
        s.kind = (uint32_t)zsrec::lister_step_w(img, size, off, w, s.rec, &s.next);
        return s;
    }
    static __device__ __forceinline__ void fold_rec(const zscrc_zs_record &r, Acc &acc)
    {
        acc.del += r.val_off == ZSCRC_ZS_DELETED;
        acc.klen += r.key_len;
        acc.vlen += r.val_len;
        acc.kmax = r.key_len > acc.kmax ? r.key_len : acc.kmax;
        acc.vmax = r.val_len > acc.vmax ? r.val_len : acc.vmax;
    }
    static __device__ __forceinline__ void store_rec(uint64_t *recs, uint64_t rank, const zscrc_zs_record &r)
    {
        uint64_t *o = recs + 4 * rank;
        o[0] = r.key_off;
        o[1] = r.key_len;
        o[2] = r.val_off;
        o[3] = r.val_len;
    }
    template <bool MULTI>
    static __device__ __forceinline__ void put(const Walk &a, const Multi &m, uint64_t rank, uint64_t, const S &s,
                                               Acc &acc)
    {
        if (rank < a.cap) {
            if constexpr (MULTI) { /* offsets into the arena; an image lies inside it: no wrap */
                zscrc_zs_record r = s.rec;
                r.key_off += m.add;
                if (r.val_off != ZSCRC_ZS_DELETED)
                    r.val_off += m.add;
                store_rec(a.off, rank, r);
            } else {
                store_rec(a.off, rank, s.rec);
            }
        }
        fold_rec(s.rec, acc);
    }
    static __device__ __forceinline__ void fold_init(uint64_t *w)
    {
        for (int i = 0; i < FOLD; ++i)
            w[i] = 0;
    }
    /* sums and maxima into w[0..4] (LDS or the result words [3..7]) */
    static __device__ __forceinline__ void fold_words(uint64_t *w, uint64_t del, uint64_t klen, uint64_t vlen,
                                                      uint64_t kmax, uint64_t vmax)
    {
        unsigned long long *u = reinterpret_cast<unsigned long long *>(w);
        if (del)
            atomicAdd(u, (unsigned long long)del);
        if (klen) {
            atomicAdd(u + 1, (unsigned long long)klen);
            atomicMax(u + 3, (unsigned long long)kmax);
        }
        if (vlen) {
            atomicAdd(u + 2, (unsigned long long)vlen);
            atomicMax(u + 4, (unsigned long long)vmax);
        }
    }
    static __device__ __forceinline__ void fold_lds(uint64_t *w, const Acc &acc)
    {
        fold_words(w, acc.del, acc.klen, acc.vlen, acc.kmax, acc.vmax);
    }
    static __device__ __forceinline__ bool folded(const uint64_t (&w)[FOLD]) { return (w[0] | w[1] | w[2]) != 0; }
    static __device__ __forceinline__ void acc_words(const Acc &acc, uint64_t (&w)[FOLD])
    {
        w[0] = acc.del;
        w[1] = acc.klen;
        w[2] = acc.vlen;
        w[3] = acc.kmax;
        w[4] = acc.vmax;
    }
    template <bool MULTI>
    static __device__ __forceinline__ void fold_out(const Walk &a, const Multi &m, uint64_t *w)
    {
        fold_words(a.res + 3, w[0], w[1], w[2], w[3], w[4]);
        if constexpr (MULTI)
            fold_words(m.tot + 2, w[0], w[1], w[2], w[3], w[4]);
    }
    /* the totals' fold words [2] .. [6], and [7]: the images that do not list to their end */
    static __device__ __forceinline__ void tot_init(uint64_t *tot, uint64_t, uint64_t bad)
    {
        for (int i = 0; i < FOLD; ++i)
            tot[2 + i] = 0;
        tot[7] = bad;
    }
    /* the emit launch folds the blocks' records into [3] .. [7] */
    static __device__ __forceinline__ void finish(const Walk &a, int rc, uint64_t n, uint64_t end, const Acc &acc,
                                                  uint64_t took_over)
    {
        a.res[0] = n > a.cap ? (uint64_t)ZSCRC_ZS_OVERFLOW : (uint64_t)rc;
        a.res[1] = n;
        a.res[2] = end;
        a.res[3] = acc.del;
        a.res[4] = acc.klen;
        a.res[5] = acc.vlen;
        a.res[6] = acc.kmax;
        a.res[7] = acc.vmax;
        a.res[8] = took_over;
        a.res[9] = a.res[10] = a.res[11] = 0;
    }
};

/* The table sweep of block `blk` of the image a describes, by one workgroup
 * (walk_table_kernel, walk_multi_table_kernel, records_table_kernel). */
template <class P>
__device__ __forceinline__ void table_sweep(const Walk &a, uint32_t blk)
{
    __shared__ uint32_t s_p[TILE_SLOTS_MAX];   /* link (slot in the tile); a root points at itself */
    __shared__ uint32_t s_acc[TILE_SLOTS_MAX]; /* S_OUT records from the slot up to its link, exclusive */
    __shared__ uint32_t s_rj[TILE_SLOTS_MAX];  /* roots: J and C of the root itself */
    __shared__ uint32_t s_rc[TILE_SLOTS_MAX];
    const uint64_t b0 = (uint64_t)blk * a.bs;
    const uint64_t bend = b0 + a.bs < a.ns ? b0 + a.bs : a.ns;
    const uint32_t tiles = (uint32_t)((bend - b0 + a.ts - 1) / a.ts);
    for (uint32_t t = tiles; t-- > 0;) {
        const uint64_t t0 = b0 + (uint64_t)t * a.ts;
        uint64_t w[SPT];
        tile_words(a, t0, bend, w);
#pragma unroll
        for (uint32_t j = 0; j < SPT; ++j) {
            const uint32_t i = threadIdx.x + j * WG;
            if (i >= a.ts)
                break;
            const uint64_t k = t0 + i;
            uint32_t p = i, acc = 0, rj = 0, rc = 0;
            if (k < bend) {
                const typename P::S s = P::step_w(a.img, a.size, k << 3, w[j]);
                const uint32_t cm = s.kind == S_OUT;
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

__global__ __launch_bounds__(WG) void walk_table_kernel(Walk a) { table_sweep<CommitWalk>(a, blockIdx.x); }

/* The plain host loop (zscrc_zs_walk, or the policy's) from off, one lane; at
 * most one step per slot.  out(offset, step) for every S_OUT record passed;
 * off ends where the walk does.  (The many-image walk counts a tail in one launch and stores
 * its spans in a later one.)  This loop and chain_hops' set rc and break:
 * with returns inside them a step and a hop took 2-3 % longer. */
template <class P, class F>
__device__ __forceinline__ int serial_loop(const Walk &a, uint64_t &off, F out)
{
    int rc = ZSCRC_ZS_END;
    for (uint64_t it = 0; it <= a.ns && off < a.size; ++it) {
        const typename P::S s = step<P>(a.img, a.size, off);
        if (s.kind == S_TRUNC) {
            rc = ZSCRC_ZS_TRUNCATED;
            break;
        }
        if (s.kind == S_STOP) {
            rc = ZSCRC_ZS_STOPPED;
            break;
        }
        if (s.kind == S_OUT)
            out(off, s);
        off = s.next;
    }
    return rc;
}

/* A single image's one-lane loop from (off, n): its output goes to index n
 * onwards, and it writes the result words. */
template <class P>
__device__ void serial_walk(const Walk &a, uint64_t off, uint64_t n, uint64_t took_over)
{
    typename P::Acc acc;
    const int rc = serial_loop<P>(a, off, [&](uint64_t at, const typename P::S &s) {
        P::template put<false>(a, Multi{}, n++, at, s, acc);
    });
    P::finish(a, rc, n, off, acc, took_over);
}

__global__ __launch_bounds__(64) void walk_serial_kernel(Walk a)
{
    if (threadIdx.x == 0 && blockIdx.x == 0)
        serial_walk<CommitWalk>(a, HDR, 0, U64_MAX);
}

/* The chain of image a, one lane: k = J[k] from slot 5, one hop per block
 * entered, each entered block's Entry written.  Returns the result code, with
 * n = the commits passed and end = the end offset; or -1 where the chain
 * reaches an offset that is no multiple of 8, unaligned (else U64_MAX), with n
 * = the commits before it: the one-lane loop goes on from there. */
template <class P>
__device__ __forceinline__ int chain_hops(const Walk &a, uint64_t &n, uint64_t &end, uint64_t &unaligned)
{
    uint64_t k = HDR / 8;
    int rc = -1; /* -1: the chain goes on */
    n = end = 0;
    unaligned = U64_MAX;
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
        const typename P::S s = step<P>(a.img, a.size, e);
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
    return rc;
}

/* A single image's chain launch, one workgroup: every entry marked as
 * skipped, then one lane hops and writes the result words.  (a by value, as
 * the kernel has it: by reference the commit instance came out three
 * instructions longer than with this body written into walk_chain_kernel.) */
template <class P>
__device__ __forceinline__ void chain_walk(const Walk a)
{
    for (uint64_t b = threadIdx.x; b < a.nblocks; b += WG)
        a.entry[b].slot = NONE;
    __syncthreads();
    if (threadIdx.x != 0)
        return;
    uint64_t n, end, unaligned;
    const int rc = chain_hops<P>(a, n, end, unaligned);
    if (unaligned != U64_MAX) {
        serial_walk<P>(a, unaligned, n, unaligned);
        return;
    }
    P::finish(a, rc, n, end, typename P::Acc{}, U64_MAX);
}

__global__ __launch_bounds__(WG) void walk_chain_kernel(Walk a) { chain_walk<CommitWalk>(a); }

/* The emit sweep of block `blk` of the image a describes, by one workgroup
 * (walk_emit_kernel, walk_multi_emit_kernel): the block's spans from index
 * first_index + the entry's base onwards, lengths folded into res[3], res[4].
 * MULTI, the many-image walk: offsets into the arena, the image's index
 * beside them, lengths folded into the totals as well (m; unused otherwise). */
template <class P, bool MULTI>
__device__ __forceinline__ void emit_sweep(const Walk &a, uint32_t blk, uint64_t first_index, const Multi &m)
{
    __shared__ uint32_t s_p[TILE_SLOTS_MAX]; /* link; after the doubling: 1 = a visited S_OUT record */
    __shared__ uint32_t s_m[TILE_SLOTS_MAX]; /* 1 = the walk visits the slot */
    __shared__ uint32_t s_scan[2][WG];
    __shared__ uint32_t s_cur;               /* the walk's next slot in the block, NONE = it left */
    __shared__ uint64_t s_mm[P::FOLD];       /* the workgroup's fold (the commit walk: longest and shortest span) */
    const Entry en = a.entry[blk];
    if (en.slot == NONE)
        return;
    const uint64_t b0 = (uint64_t)blk * a.bs;
    const uint64_t bend = b0 + a.bs < a.ns ? b0 + a.bs : a.ns;
    const uint32_t tiles = (uint32_t)((bend - b0 + a.ts - 1) / a.ts);
    const uint32_t per = a.ts > WG ? a.ts / WG : 1; /* slots per thread of the scan, contiguous */
    uint64_t base = first_index + en.base;
    typename P::Acc acc;
    if (threadIdx.x == 0) {
        s_cur = en.slot;
        P::fold_init(s_mm);
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
        tile_words(a, t0, bend, w);
#pragma unroll
        for (uint32_t j = 0; j < SPT; ++j) {
            const uint32_t i = threadIdx.x + j * WG;
            if (i >= a.ts)
                break;
            const uint64_t k = t0 + i;
            uint32_t p = i;
            if (k < bend) {
                const uint64_t n = link_of(P::step_w(a.img, a.size, k << 3, w[j]), tend);
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
                const typename P::S s = step<P>(a.img, a.size, (t0 + i) << 3);
                f = s.kind == S_OUT;
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
        uint32_t total;
        uint64_t rank = base + tile_scan(s_scan, mine, total) - mine;
        if (mine) {
            for (uint32_t j = 0; j < per; ++j) {
                if (!s_p[first + j])
                    continue;
                const uint64_t off = (t0 + first + j) << 3;
                const typename P::S s = step<P>(a.img, a.size, off);
                P::template put<MULTI>(a, m, rank++, off, s, acc);
            }
        }
        base += total;
        __syncthreads(); /* s_p, s_scan and s_cur are rewritten by the next tile */
    }
    P::fold_lds(s_mm, acc);
    __syncthreads();
    const bool any = P::folded(s_mm);
    if (threadIdx.x == 0 && any)
        P::template fold_out<MULTI>(a, m, s_mm);
}

__global__ __launch_bounds__(WG) void walk_emit_kernel(Walk a)
{
    emit_sweep<CommitWalk, false>(a, blockIdx.x, 0, Multi{});
}

/* ------------------------------------------------------- the record lister
 * zscrc_device_records, active and finalised images: the three launches above
 * (or the one-lane loop) as instances of RecordList. */
__global__ __launch_bounds__(WG) void records_table_kernel(Walk a) { table_sweep<RecordList>(a, blockIdx.x); }

__global__ __launch_bounds__(64) void records_serial_kernel(Walk a)
{
    if (threadIdx.x == 0 && blockIdx.x == 0)
        serial_walk<RecordList>(a, HDR, 0, U64_MAX);
}

__global__ __launch_bounds__(WG) void records_chain_kernel(Walk a) { chain_walk<RecordList>(a); }

__global__ __launch_bounds__(WG) void records_emit_kernel(Walk a)
{
    emit_sweep<RecordList, false>(a, blockIdx.x, 0, Multi{});
}

/* Packed images: the records in pointer-section order.  There is no chain --
 * pointer i is parsed on its own -- but the host lister stops at the first
 * pointer whose record does not parse, so the smallest failing index is found
 * first (an integer min) and only the records before it are put out; record i
 * is output entry i.
 *
 *   records_packed_locate_kernel  one lane: the two spans (packed_spans) and
 *                                 the pointer count; the result words
 *   records_packed_find_kernel    one pointer per thread, grid-stride: the
 *                                 smallest index whose record does not parse
 *   records_packed_emit_kernel    one pointer per thread, grid-stride, below
 *                                 that index: stores and folds; res[0], res[1]
 */
struct Packed {
    const uint8_t *img;
    uint64_t size;
    uint64_t *recs;
    uint64_t cap;
    uint64_t *res;
    uint64_t *sc; /* scratch: PK_WORDS words */
};
/* PK_FAIL: the first pointer that does not parse, the count where all do */
enum { PK_POFF = 0, PK_COUNT = 1, PK_FAIL = 2, PK_WORDS = 8 };
constexpr unsigned PACKED_GRID_MAX = 2048;

__global__ __launch_bounds__(64) void records_packed_locate_kernel(Packed a)
{
    if (threadIdx.x != 0 || blockIdx.x != 0)
        return;
    uint64_t so[2], sl[2], poff = 0, count = 0;
    int rc = zsrec::packed_spans(zsrec::Direct{a.img}, a.size, so, sl);
    if (rc == ZSCRC_OK) {
        poff = so[1];
        if (!zsrec::pointer_count(a.img, poff, sl[1], &count)) {
            rc = ZSCRC_ZS_TRUNCATED;
            count = 0;
        }
    }
    a.sc[PK_POFF] = poff;
    a.sc[PK_COUNT] = count;
    a.sc[PK_FAIL] = count;
    /* as the host returns it: no record listed where the sections are not
     * found; the emit launch writes [0] and [1] where there are pointers */
    a.res[0] = (uint64_t)(int64_t)rc;
    a.res[1] = 0;
    a.res[2] = poff;
    for (int i = 3; i < ZSCRC_RECORDS_RES_WORDS; ++i)
        a.res[i] = 0;
    a.res[8] = U64_MAX;
}

__global__ __launch_bounds__(WG) void records_packed_find_kernel(Packed a)
{
    const uint64_t poff = a.sc[PK_POFF], count = a.sc[PK_COUNT];
    const uint64_t stride = (uint64_t)gridDim.x * WG;
    uint64_t fail = U64_MAX;
    /* ascending: a thread's first failure is its smallest */
    for (uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x; i < count && fail == U64_MAX; i += stride) {
        zscrc_zs_record r;
        uint64_t next;
        if (!zsrec::record_at(a.img, a.size, zsrec::pointer_at(a.img, poff, i), r, &next))
            fail = i;
    }
    if (fail != U64_MAX)
        atomicMin(reinterpret_cast<unsigned long long *>(a.sc + PK_FAIL), (unsigned long long)fail);
}

__global__ __launch_bounds__(WG) void records_packed_emit_kernel(Packed a)
{
    __shared__ uint64_t s_fold[RecordList::FOLD];
    const uint64_t poff = a.sc[PK_POFF], count = a.sc[PK_COUNT], n = a.sc[PK_FAIL];
    const uint64_t stride = (uint64_t)gridDim.x * WG;
    if (threadIdx.x == 0)
        RecordList::fold_init(s_fold);
    __syncthreads();
    RecordList::Acc acc;
    for (uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x; i < n; i += stride) {
        zscrc_zs_record r;
        uint64_t next;
        /* parses: i is below the first index that does not */
        if (!zsrec::record_at(a.img, a.size, zsrec::pointer_at(a.img, poff, i), r, &next))
            continue;
        if (i < a.cap)
            RecordList::store_rec(a.recs, i, r);
        RecordList::fold_rec(r, acc);
    }
    RecordList::fold_lds(s_fold, acc);
    __syncthreads();
    if (threadIdx.x != 0)
        return;
    RecordList::fold_words(a.res + 3, s_fold[0], s_fold[1], s_fold[2], s_fold[3], s_fold[4]);
    if (blockIdx.x == 0 && count) {
        a.res[0] = n > a.cap ? (uint64_t)ZSCRC_ZS_OVERFLOW : n < count ? (uint64_t)ZSCRC_ZS_TRUNCATED : 0;
        a.res[1] = n;
    }
}

/* ------------------------------------------------- many images of one arena
 * zscrc_device_walk_multi: the same walk over k images of one device buffer
 * in four launches whatever k is.  Every image is cut into slots and blocks
 * from its own first byte, so J, C and the entries of image j are exactly the
 * single walk's for those bytes; the blocks (and slots) of all images are
 * numbered one after another, image j's from blk0 (slot0) of its descriptor.
 *
 *   walk_multi_table_kernel  one workgroup per (image, block): table_sweep of
 *                            that block; marks the block's entry as skipped
 *   walk_multi_chain_kernel  one lane per image: chain_hops over its own J and
 *                            entries; row words [0] [1] [2] [5], the
 *                            initial [3] [4]; past an unaligned next offset it
 *                            only counts (serial_loop)
 *   walk_multi_scan_kernel   one workgroup: row[6] = exclusive prefix sum of
 *                            the counts (scan_counts, zscrc_wg.h); totals
 *   walk_multi_emit_kernel   one workgroup per (image, block): emit_sweep from
 *                            row[6]; and one lane per image that walks a
 *                            counted tail again, storing its spans
 *
 * zscrc_device_records_multi is the same four launches with the RecordList
 * policy (records_multi_*_kernel): each family is multi_table / multi_chain /
 * multi_scan / multi_emit below with its policy, which also names the row's
 * layout (P::ROW words; P::TAKE the take-over word, [5] above; P::FIRST the
 * first-index word, [6] above).  The records family sweeps tables of its own.
 * A counted tail is folded in the emit launch only, where it is stored.
 */
struct ImgD {
    uint64_t off, size;   /* the image: bytes [off, off + size) of the arena */
    uint64_t slot0;       /* its first slot of J and C */
    uint32_t blk0;        /* its first block; blocks: blk0 of the next descriptor - blk0 */
    uint32_t pad;
};

struct MWalk {
    const uint8_t *arena;
    const ImgD *im;       /* scratch: k + 1, the last one holds the totals */
    uint64_t *tail_n;     /* scratch: k, the commits (records) before a counted tail */
    Entry *entry;         /* scratch: every image's blocks */
    uint32_t *J, *C;      /* scratch: every image's slots */
    uint32_t k, nblocks;
    uint32_t bs, ts, rounds;
    uint64_t *off, *len;  /* the spans (the record lister: off = the entries, four words each; len, img unused) */
    uint32_t *img;
    uint64_t cap;
    uint64_t *rows, *tot; /* k rows of P::ROW words; the totals */
};

constexpr uint64_t MULTI_MAX = ZSCRC_WALK_MULTI_MAX;
constexpr int ROW = ZSCRC_WALK_ROW_WORDS;

/* The image that block blk (< nblocks) belongs to: the last j with
 * im[j].blk0 <= blk (images without blocks share their blk0 with the next
 * one).  Uniform over the workgroup; at most 21 probes. */
__device__ __forceinline__ uint32_t image_of(const MWalk &a, uint32_t blk)
{
    uint32_t lo = 0, hi = a.k; /* im[lo].blk0 <= blk < im[hi].blk0 */
    for (int it = 0; it < 21 && hi - lo > 1; ++it) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.im[mid].blk0 <= blk)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

/* Image j as the single walk of policy P sees it; its output goes to the
 * shared arrays, its result words to its row. */
template <class P>
__device__ __forceinline__ Walk view_of(const MWalk &a, uint32_t j)
{
    const ImgD d = a.im[j];
    Walk w;
    w.img = a.arena + d.off;
    w.size = d.size;
    w.ns = d.size / 8 + (d.size % 8 != 0);
    w.bs = a.bs;
    w.ts = a.ts;
    w.rounds = a.rounds;
    w.nblocks = a.im[j + 1].blk0 - d.blk0;
    w.entry = a.entry + d.blk0;
    w.J = a.J + d.slot0;
    w.C = a.C + d.slot0;
    w.off = a.off;
    w.len = a.len;
    w.cap = a.cap;
    w.res = a.rows + (uint64_t)j * P::ROW;
    return w;
}

template <class P>
__device__ __forceinline__ void multi_table(const MWalk &a)
{
    const uint32_t j = image_of(a, blockIdx.x);
    const Walk w = view_of<P>(a, j);
    const uint32_t blk = blockIdx.x - a.im[j].blk0;
    if (threadIdx.x == 0)
        w.entry[blk].slot = NONE;
    table_sweep<P>(w, blk);
}

/* One lane per image: the row as P::finish writes the result words of that
 * image alone with unlimited room (so [0] is never OVERFLOW), the fold words
 * at their initial values; the words after P::FIRST 0. */
template <class P>
__device__ __forceinline__ void multi_chain(const MWalk &a)
{
    const uint64_t j = (uint64_t)blockIdx.x * WG + threadIdx.x;
    if (j >= a.k)
        return;
    Walk w = view_of<P>(a, (uint32_t)j);
    w.cap = U64_MAX;
    for (int i = P::FIRST + 1; i < P::ROW; ++i)
        w.res[i] = 0;
    if (w.size < HDR) { /* nothing to walk: the host loop's ZSCRC_EINVAL */
        P::finish(w, ZSCRC_EINVAL, 0, 0, typename P::Acc{}, U64_MAX);
        return;
    }
    uint64_t n, end, unaligned;
    int rc = chain_hops<P>(w, n, end, unaligned);
    a.tail_n[j] = n;
    if (unaligned != U64_MAX) { /* the output positions are not known yet: count */
        end = unaligned;
        rc = serial_loop<P>(w, end, [&n](uint64_t, const typename P::S &) { ++n; });
    }
    P::finish(w, rc, n, end, typename P::Acc{}, unaligned);
}

/* One workgroup: row[P::FIRST] = exclusive prefix sum of the counts
 * (scan_counts, zscrc_wg.h); the totals, their fold words at the initial
 * values the emit launch folds into. */
template <class P>
__device__ __forceinline__ void multi_scan(const MWalk &a)
{
    __shared__ uint64_t s_scan[WG / 64];
    const uint64_t carry = scan_counts(
        s_scan, a.k, [&a](uint64_t i) { return a.rows[i * P::ROW + 1]; },
        [&a](uint64_t i, uint64_t at) { a.rows[i * P::ROW + P::FIRST] = at; });
    uint64_t bad = 0; /* images whose row [0] is not END, where the totals have a word for them */
    if constexpr (P::TOT_NOT_END) {
        for (uint64_t i = threadIdx.x; i < a.k; i += WG)
            bad += a.rows[i * P::ROW] != (uint64_t)ZSCRC_ZS_END;
        bad = wg_sum(s_scan, bad);
    }
    if (threadIdx.x == 0) {
        a.tot[0] = carry > a.cap ? (uint64_t)ZSCRC_ZS_OVERFLOW : 0;
        a.tot[1] = carry;
        P::tot_init(a.tot, carry, bad);
    }
}

/* Workgroup w: the emit sweep of block w (if there is one), then one lane per
 * image of [w * WG, w * WG + WG) for the counted tails (if there are such
 * images): a grid of max(blocks, ceil(k / WG)) workgroups.  A tail's records
 * are stored from row[P::FIRST] + the records before the tail, and folded
 * here and nowhere else. */
template <class P>
__device__ __forceinline__ void multi_emit(const MWalk &a)
{
    if (blockIdx.x < a.nblocks) {
        const uint32_t j = image_of(a, blockIdx.x);
        const Walk w = view_of<P>(a, j);
        emit_sweep<P, true>(w, blockIdx.x - a.im[j].blk0, w.res[P::FIRST], Multi{a.im[j].off, a.img, j, a.tot});
    }
    const uint64_t j = (uint64_t)blockIdx.x * WG + threadIdx.x;
    if (j >= a.k || a.rows[j * P::ROW + P::TAKE] == U64_MAX)
        return;
    const Walk w = view_of<P>(a, (uint32_t)j);
    const Multi m{a.im[j].off, a.img, (uint32_t)j, a.tot};
    uint64_t off = w.res[P::TAKE], n = w.res[P::FIRST] + a.tail_n[j];
    typename P::Acc acc;
    (void)serial_loop<P>(w, off, [&](uint64_t at, const typename P::S &s) {
        P::template put<true>(w, m, n++, at, s, acc);
    });
    uint64_t f[P::FOLD];
    P::acc_words(acc, f);
    if (P::folded(f))
        P::template fold_out<true>(w, m, f);
}

__global__ __launch_bounds__(WG) void walk_multi_table_kernel(MWalk a) { multi_table<CommitWalk>(a); }
__global__ __launch_bounds__(WG) void walk_multi_chain_kernel(MWalk a) { multi_chain<CommitWalk>(a); }
__global__ __launch_bounds__(WG) void walk_multi_scan_kernel(MWalk a) { multi_scan<CommitWalk>(a); }
__global__ __launch_bounds__(WG) void walk_multi_emit_kernel(MWalk a) { multi_emit<CommitWalk>(a); }

/* zscrc_device_records_multi: off = the record entries of all images (four
 * words each), len and img unused, rows of ZSCRC_RECORDS_ROW_WORDS words. */
__global__ __launch_bounds__(WG) void records_multi_table_kernel(MWalk a) { multi_table<RecordList>(a); }
__global__ __launch_bounds__(WG) void records_multi_chain_kernel(MWalk a) { multi_chain<RecordList>(a); }
__global__ __launch_bounds__(WG) void records_multi_scan_kernel(MWalk a) { multi_scan<RecordList>(a); }
__global__ __launch_bounds__(WG) void records_multi_emit_kernel(MWalk a) { multi_emit<RecordList>(a); }

/* The 40-byte headers of k images, one after another (zscrc_device_verify_images);
 * zeros for an image of fewer than 40 bytes. */
__global__ __launch_bounds__(WG) void walk_multi_headers_kernel(const uint8_t *arena, const ImgD *im, uint32_t k,
                                                                uint8_t *out)
{
    const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
    if (i >= (uint64_t)k * HDR)
        return;
    const ImgD d = im[i / HDR];
    out[i] = d.size >= HDR ? arena[d.off + i % HDR] : 0;
}

/* ------------------------------------------------------------------ host */

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

/* records: the record lister's instances instead of the commit walk's. */
int launch(const Walk &w, unsigned flags, hipStream_t s, bool records)
{
    const dim3 blocks((unsigned)w.nblocks);
    if (serial_only(w, flags)) {
        hipLaunchKernelGGL(records ? records_serial_kernel : walk_serial_kernel, dim3(1), dim3(64), 0, s, w);
    } else {
        hipLaunchKernelGGL(records ? records_table_kernel : walk_table_kernel, blocks, dim3(WG), 0, s, w);
        hipLaunchKernelGGL(records ? records_chain_kernel : walk_chain_kernel, dim3(1), dim3(WG), 0, s, w);
        hipLaunchKernelGGL(records ? records_emit_kernel : walk_emit_kernel, blocks, dim3(WG), 0, s, w);
    }
    return hipGetLastError() == hipSuccess ? ZSCRC_OK : ZSCRC_EHIP;
}

/* The walk of one image (w: geometry, image, output and result pointers set)
 * with the caller's scratch or, scratch == NULL, the library's. */
int walk_single(Walk &w, void *scratch, unsigned flags, hipStream_t s, bool records)
{
    if (serial_only(w, flags)) /* touches no scratch */
        return launch(w, flags, s, records);
    return zs::with_scratch(scratch, scratch_bytes(w), false, s, [&](void *p, Scratch *) {
        w.entry = static_cast<Entry *>(p);
        w.J = reinterpret_cast<uint32_t *>(w.entry + w.nblocks);
        w.C = w.J + w.ns;
        return launch(w, flags, s, records);
    });
}

int launch_packed(const Packed &a, unsigned flags, hipStream_t s)
{
    /* the pointer count is on the device only: a grid for the most the image
     * can hold (one pointer per 8 bytes), capped; the kernels stride */
    uint64_t g = a.size / 8 / WG + 1;
    if (g > PACKED_GRID_MAX || (flags & ZSCRC_WALK_SERIAL))
        g = (flags & ZSCRC_WALK_SERIAL) ? 1 : PACKED_GRID_MAX;
    hipLaunchKernelGGL(records_packed_locate_kernel, dim3(1), dim3(64), 0, s, a);
    hipLaunchKernelGGL(records_packed_find_kernel, dim3((unsigned)g), dim3(WG), 0, s, a);
    hipLaunchKernelGGL(records_packed_emit_kernel, dim3((unsigned)g), dim3(WG), 0, s, a);
    return hipGetLastError() == hipSuccess ? ZSCRC_OK : ZSCRC_EHIP;
}

/* The many-image walk's geometry and scratch layout: the descriptors (k + 1),
 * the counts before a tail (k), then entries, J and C of all images. */
struct Plan {
    uint32_t bs, ts, rounds;
    uint64_t nslots, nblocks;
    size_t tail_at, entry_at, j_at, c_at, bytes;
};

uint64_t slots_of(uint64_t size) { return size < HDR ? 0 : size / 8 + (size % 8 != 0); }

/* false = bad arguments.  check_arena: every image must lie inside
 * arena_size bytes.  desc (k + 1 entries, may be NULL) receives the
 * descriptors. */
bool plan_multi(const zscrc_walk_image *images, size_t k, bool check_arena, uint64_t arena_size,
                const zscrc_walk_opts *o, Plan *p, ImgD *desc)
{
    Walk g{};
    if (!images || k == 0 || k > MULTI_MAX || !geometry(0, o, &g))
        return false;
    p->bs = g.bs;
    p->ts = g.ts;
    p->rounds = g.rounds;
    uint64_t slots = 0, blocks = 0;
    for (size_t j = 0; j < k; ++j) {
        const uint64_t off = images[j].off, size = images[j].size;
        if (size > U64_MAX - off) /* no arena holds it */
            return false;
        if (check_arena && (off > arena_size || size > arena_size - off))
            return false;
        if (desc)
            desc[j] = ImgD{off, size, slots, (uint32_t)blocks, 0};
        const uint64_t ns = slots_of(size);
        slots += ns; /* < 2^61 each, k <= 2^20: no wrap */
        blocks += (ns + g.bs - 1) / g.bs;
        if (blocks > BLOCKS_MAX) /* one workgroup per block: a grid's threads must stay below 2^32 */
            return false;
    }
    if (desc)
        desc[k] = ImgD{0, 0, slots, (uint32_t)blocks, 0};
    p->nslots = slots;
    p->nblocks = blocks;
    p->tail_at = (k + 1) * sizeof(ImgD);
    p->entry_at = p->tail_at + up16(k * 8);
    p->j_at = p->entry_at + (size_t)blocks * sizeof(Entry);
    p->c_at = p->j_at + (size_t)slots * 4;
    p->bytes = p->c_at + (size_t)slots * 4;
    return true;
}

/* With sc.mu held: the descriptors of `images` copied to d_desc (device,
 * k + 1 entries) in stream order, through the pinned staging. */
int stage_descriptors(Scratch &sc, const zscrc_walk_image *images, size_t k, const zscrc_walk_opts *o,
                      void *d_desc, hipStream_t s)
{
    const size_t bytes = (k + 1) * sizeof(ImgD);
    const int rc = zs::stage_begin(sc, bytes);
    if (rc)
        return rc;
    Plan p;
    if (!plan_multi(images, k, false, 0, o, &p, sc.pin.as<ImgD>()))
        return ZSCRC_EINVAL;
    return zs::stage_copy(sc, d_desc, bytes, s);
}

/* records: the record lister's instances instead of the commit walk's. */
int launch_multi(const MWalk &m, hipStream_t s, bool records)
{
    const unsigned lanes = (m.k + WG - 1) / WG;
    if (m.nblocks)
        hipLaunchKernelGGL(records ? records_multi_table_kernel : walk_multi_table_kernel, dim3(m.nblocks), dim3(WG),
                           0, s, m);
    hipLaunchKernelGGL(records ? records_multi_chain_kernel : walk_multi_chain_kernel, dim3(lanes), dim3(WG), 0, s, m);
    hipLaunchKernelGGL(records ? records_multi_scan_kernel : walk_multi_scan_kernel, dim3(1), dim3(WG), 0, s, m);
    hipLaunchKernelGGL(records ? records_multi_emit_kernel : walk_multi_emit_kernel,
                       dim3(m.nblocks > lanes ? m.nblocks : lanes), dim3(WG), 0, s, m);
    return hipGetLastError() == hipSuccess ? ZSCRC_OK : ZSCRC_EHIP;
}

/* The many-image call of either family (m: arena, outputs, rows and totals
 * set): geometry and scratch pointers from the plan, the descriptors staged,
 * the four launches. */
int walk_multi(MWalk &m, const Plan &p, const zscrc_walk_image *images, size_t k, void *scratch,
               const zscrc_walk_opts *opts, hipStream_t s, bool records)
{
    m.k = (uint32_t)k;
    m.nblocks = (uint32_t)p.nblocks;
    m.bs = p.bs;
    m.ts = p.ts;
    m.rounds = p.rounds;
    return zs::with_scratch(scratch, p.bytes, true, s, [&](void *sp, Scratch *sc) {
        uint8_t *base = static_cast<uint8_t *>(sp);
        m.im = reinterpret_cast<const ImgD *>(base);
        m.tail_n = reinterpret_cast<uint64_t *>(base + p.tail_at);
        m.entry = reinterpret_cast<Entry *>(base + p.entry_at);
        m.J = reinterpret_cast<uint32_t *>(base + p.j_at);
        m.C = reinterpret_cast<uint32_t *>(base + p.c_at);
        const int rc = stage_descriptors(*sc, images, k, opts, base, s);
        return rc ? rc : launch_multi(m, s, records);
    });
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
    return walk_single(w, scratch, flags, static_cast<hipStream_t>(stream), false);
}

size_t zscrc_device_records_scratch_bytes(uint64_t image_size, int kind, const zscrc_walk_opts *opts)
{
    Walk w{};
    if ((kind != ZSCRC_ZS_ACTIVE && kind != ZSCRC_ZS_FINALISED && kind != ZSCRC_ZS_PACKED) ||
        !geometry(image_size, opts, &w))
        return 0;
    return kind == ZSCRC_ZS_PACKED ? PK_WORDS * sizeof(uint64_t) : scratch_bytes(w);
}

int zscrc_device_records(const void *d_image, uint64_t image_size, int kind, struct zscrc_zs_record *d_recs,
                         size_t cap, uint64_t *d_res, void *scratch, const zscrc_walk_opts *opts, unsigned flags,
                         void *stream)
{
    Walk w{};
    const bool packed = kind == ZSCRC_ZS_PACKED;
    if (!d_image || !d_res || (cap && !d_recs) || (flags & ~ZSCRC_WALK_SERIAL) ||
        (kind != ZSCRC_ZS_ACTIVE && kind != ZSCRC_ZS_FINALISED && !packed) ||
        image_size < (packed ? HDR + 16 : HDR) || !geometry(image_size, opts, &w) ||
        (reinterpret_cast<uintptr_t>(scratch) & 15))
        return ZSCRC_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!packed) {
        w.img = static_cast<const uint8_t *>(d_image);
        w.off = reinterpret_cast<uint64_t *>(d_recs); /* four words an entry (RecordList) */
        w.len = nullptr;
        w.cap = cap;
        w.res = d_res;
        return walk_single(w, scratch, flags, s, true);
    }
    Packed a{static_cast<const uint8_t *>(d_image), image_size, reinterpret_cast<uint64_t *>(d_recs), cap, d_res,
             static_cast<uint64_t *>(scratch)};
    return zs::with_scratch(scratch, PK_WORDS * sizeof(uint64_t), false, s, [&](void *p, Scratch *) {
        a.sc = static_cast<uint64_t *>(p);
        return launch_packed(a, flags, s);
    });
}

size_t zscrc_device_walk_multi_scratch_bytes(const zscrc_walk_image *images, size_t k, const zscrc_walk_opts *opts)
{
    Plan p;
    return plan_multi(images, k, false, 0, opts, &p, nullptr) ? p.bytes : 0;
}

int zscrc_device_walk_multi(const void *d_arena, uint64_t arena_size, const zscrc_walk_image *images, size_t k,
                            uint64_t *d_span_off, uint64_t *d_span_len, uint32_t *d_span_img, size_t cap,
                            uint64_t *d_rows, uint64_t *d_tot, void *scratch, const zscrc_walk_opts *opts,
                            unsigned flags, void *stream)
{
    Plan p;
    if (!d_arena || !d_rows || !d_tot || (cap && (!d_span_off || !d_span_len || !d_span_img)) || flags ||
        (reinterpret_cast<uintptr_t>(scratch) & 15) || !plan_multi(images, k, true, arena_size, opts, &p, nullptr))
        return ZSCRC_EINVAL;
    MWalk m{};
    m.arena = static_cast<const uint8_t *>(d_arena);
    m.off = d_span_off;
    m.len = d_span_len;
    m.img = d_span_img;
    m.cap = cap;
    m.rows = d_rows;
    m.tot = d_tot;
    return walk_multi(m, p, images, k, scratch, opts, static_cast<hipStream_t>(stream), false);
}

size_t zscrc_device_records_multi_scratch_bytes(const zscrc_walk_image *images, size_t k,
                                                const zscrc_walk_opts *opts)
{
    return zscrc_device_walk_multi_scratch_bytes(images, k, opts);
}

int zscrc_device_records_multi(const void *d_arena, uint64_t arena_size, const zscrc_walk_image *images, size_t k,
                               struct zscrc_zs_record *d_recs, size_t cap, uint64_t *d_rows, uint64_t *d_tot,
                               void *scratch, const zscrc_walk_opts *opts, unsigned flags, void *stream)
{
    Plan p;
    if (!d_arena || !d_rows || !d_tot || (cap && !d_recs) || flags || (reinterpret_cast<uintptr_t>(scratch) & 15) ||
        !plan_multi(images, k, true, arena_size, opts, &p, nullptr))
        return ZSCRC_EINVAL;
    MWalk m{};
    m.arena = static_cast<const uint8_t *>(d_arena);
    m.off = reinterpret_cast<uint64_t *>(d_recs); /* four words an entry (RecordList) */
    m.cap = cap;
    m.rows = d_rows;
    m.tot = d_tot;
    return walk_multi(m, p, images, k, scratch, opts, static_cast<hipStream_t>(stream), true);
}

int zscrc_device_verify_images(const void *d_arena, uint64_t arena_size, const zscrc_walk_image *images, size_t k,
                               zscrc_zs_report *reps, void *stream)
{
    Plan p;
    if (!d_arena || !reps || !plan_multi(images, k, true, arena_size, nullptr, &p, nullptr))
        return ZSCRC_EINVAL;
    memset(reps, 0, k * sizeof *reps);
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch *sc = zs::device_scratch();
    if (!sc)
        return ZSCRC_ENODEV;
    /* device: descriptors, the rows, the totals, the gathered headers; host:
     * the headers, then the rows */
    const size_t desc_bytes = (k + 1) * sizeof(ImgD), rows_bytes = k * ROW * 8, hdr_bytes = k * HDR;
    /* freed at the return, after the last synchronise: dspan, then dfix */
    zs::ScopedBuf<zs::Device> dfix_buf, dspan;
    uint8_t *host = static_cast<uint8_t *>(malloc(rows_bytes > hdr_bytes ? rows_bytes : hdr_bytes));
    uint32_t *st = nullptr;
    uint64_t tot[ZSCRC_WALK_TOT_WORDS] = {};
    size_t cap = 0;
    int rc = host ? ZSCRC_OK : ZSCRC_ENOMEM;
    if (!rc)
        rc = dfix_buf.reserve(desc_bytes + rows_bytes + 64 + hdr_bytes);
    uint8_t *const dfix = dfix_buf.as<uint8_t>();
    uint64_t *drows = reinterpret_cast<uint64_t *>(dfix + desc_bytes), *dtot = drows + k * ROW;
    uint8_t *dhdr = dfix + desc_bytes + rows_bytes + 64;
    if (!rc) {
        std::lock_guard<std::mutex> lk(sc->mu);
        rc = stage_descriptors(*sc, images, k, nullptr, dfix, s);
    }
    if (!rc) {
        hipLaunchKernelGGL(walk_multi_headers_kernel, dim3((unsigned)((hdr_bytes + WG - 1) / WG)), dim3(WG), 0, s,
                           static_cast<const uint8_t *>(d_arena), reinterpret_cast<const ImgD *>(dfix), (uint32_t)k,
                           dhdr);
        if (hipGetLastError() != hipSuccess ||
            hipMemcpyAsync(host, dhdr, hdr_bytes, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
            rc = ZSCRC_EHIP;
    }
    if (!rc) {
        for (size_t j = 0; j < k; ++j) {
            const uint64_t size = images[j].size;
            reps[j].header_rc = zscrc_zs_header_crc(host + j * HDR, size >= HDR ? HDR : size, &reps[j].header_stored,
                                                    &reps[j].header_computed);
            cap += (size_t)(size / 64) + 1;
        }
    }
    /* most images hold far fewer commits than one per 8 bytes: a first walk
     * with room for one per 64 bytes, and only if that overflows a second
     * one with room for the count the first one found.  A commit slot:
     * offset, length, image, CRC, status. */
    uint64_t *doff = nullptr;
    uint32_t *dimg = nullptr;
    for (int pass = 0; !rc && pass < 2; ++pass) {
        /* the second pass frees the first one's, then allocates */
        if ((rc = dspan.reserve(cap * 28)))
            break;
        doff = dspan.as<uint64_t>();
        dimg = reinterpret_cast<uint32_t *>(doff + 2 * cap);
        rc = zscrc_device_walk_multi(d_arena, arena_size, images, k, doff, doff + cap, dimg, cap, drows, dtot, nullptr,
                                     nullptr, 0, s);
        if (!rc && (hipMemcpyAsync(tot, dtot, sizeof tot, hipMemcpyDeviceToHost, s) != hipSuccess ||
                    hipStreamSynchronize(s) != hipSuccess))
            rc = ZSCRC_EHIP;
        if (rc || tot[1] <= cap)
            break;
        cap = (size_t)tot[1];
    }
    const size_t n = (size_t)tot[1];
    if (!rc && n) {
        uint32_t *dcrc = dimg + cap, *dst = dcrc + cap;
        st = static_cast<uint32_t *>(malloc(n * 4));
        if (!st)
            rc = ZSCRC_ENOMEM;
        if (!rc)
            rc = zscrc_device_verify_commits_bounded(d_arena, arena_size, doff, doff + cap, nullptr, n, tot[2], dcrc,
                                                     dst, s);
        if (!rc && hipMemcpyAsync(st, dst, n * 4, hipMemcpyDeviceToHost, s) != hipSuccess)
            rc = ZSCRC_EHIP;
    }
    if (!rc && (hipMemcpyAsync(host, drows, rows_bytes, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipStreamSynchronize(s) != hipSuccess))
        rc = ZSCRC_EHIP;
    if (!rc) {
        const uint64_t *rows = reinterpret_cast<const uint64_t *>(host);
        for (size_t j = 0; j < k; ++j) {
            const uint64_t *row = rows + j * ROW;
            zscrc_zs_report &r = reps[j];
            r.walk_rc = (int)(int64_t)row[0];
            r.n_commits = row[1];
            r.end_off = row[2];
            /* a count the compiler vectorises, then the first: one by one, 3.35 M statuses took 0.42 or
             * 0.69 ms depending on the address the loop was placed at */
            const uint32_t *sj = st + row[6];
            uint64_t bad = 0;
            for (uint64_t i = 0; i < row[1]; ++i)
                bad += sj[i] != 1;
            r.n_bad = bad;
            if (bad) /* one of the row[1] statuses is not 1: the search ends among them */
                while (sj[r.first_bad] == 1)
                    r.first_bad++;
        }
    }
    free(st);
    free(host);
    return rc;
}

} /* extern "C" */
