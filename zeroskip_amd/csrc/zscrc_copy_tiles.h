/*
 * zscrc_copy_tiles.h -- the tile sweep of pack_copy_kernel (zscrc_devpack.hip)
 * and log_copy_kernel (zscrc_devlog.hip).  The file offsets [base, stop) that
 * hold the records are cut into tiles of T bytes, so every 16-byte word of a
 * tile is aligned in a 16-byte aligned output; a workgroup takes a run of
 * tiles, finds its first record by bisection, keeps the starts of a tile's
 * records in LDS, and every thread builds whole 16-byte words out of generated
 * words and gathered source bytes (zscrc_pack_layout.h).  Template parameters:
 *   ORIGIN  the starts are file offsets minus ORIGIN: region coordinates behind
 *           the 40-byte header for the packer (HDR), file offsets for the log (0)
 *   GAPS    commit records lie between the records and are not the sweep's to
 *           write (the log); without it the records fill [base, stop)
 * The first part has no HIP type in it: the run, the word and the advance also
 * run in a CPU program, the lanes played by a loop (tests/c/copy_tiles_sweep.h).
 */
#ifndef ZSCRC_COPY_TILES_H
#define ZSCRC_COPY_TILES_H

#include <stdint.h>

#include "zscrc_log_layout.h"
#ifdef __HIPCC__
#include "zscrc_wg.h" /* for copy_tiles, the device part */
#endif

namespace zstile {

using zspack::find_rec;
constexpr uint64_t DEF_TILE = 65536, TILE_MIN = 64, TILE_MAX = 65536;
constexpr uint32_t COPY_WG = 256; /* the threads of a copy's workgroup: zsdev::WG */
/* starts of a tile's records in LDS: the most records that reach into a tile
 * (24 bytes each at least; commit records in between only make them fewer),
 * one more for the end, rounded up to whole rounds of COPY_WG loads */
constexpr uint32_t LDS_STARTS = ((uint32_t)(TILE_MAX / 24) + 3 + COPY_WG - 1) / COPY_WG * COPY_WG + COPY_WG;
static_assert(LDS_STARTS >= TILE_MAX / 24 + 3 && LDS_STARTS % COPY_WG == 0, "the largest tile's starts, whole rounds");
/* what the 24 KiB of starts admit on a CU: every workgroup of the copy is
 * resident, so the equal runs of tiles end together.  (An instance with 8 KiB
 * of starts for tiles up to 16 KiB, eight workgroups a CU, was measured and
 * was no faster there: DESIGN.md 2.6.) */
constexpr unsigned COPY_WG_PER_CU = 6;

/* The run of tiles [t0, t1) of workgroup b of g: the tiles [t * T, (t + 1) * T)
 * that [base, stop) touches in equal runs; empty (t0 >= t1) behind the last. */
struct Run { uint64_t t0, t1; };
ZSREC_HD inline Run run_of(uint64_t b, uint64_t g, uint64_t T, uint64_t base, uint64_t stop)
{
    const uint64_t tlo = base / T, thi = (stop + T - 1) / T, per = (thi - tlo + g - 1) / g, t0 = tlo + b * per;
    return Run{t0, t0 + per < thi ? t0 + per : thi};
}
/* The first offset of tile t that is the sweep's (a run that begins with t
 * looks up its first record there), and the tile's end. */
ZSREC_HD inline uint64_t tile_lo(uint64_t t, uint64_t T, uint64_t base) { return t * T > base ? t * T : base; }
ZSREC_HD inline uint64_t tile_hi(uint64_t t, uint64_t T, uint64_t stop) { return t * T + T < stop ? t * T + T : stop; }

/* The word at rel of record r: generated, or gathered from the source. */
ZSREC_HD inline uint64_t record_word(const uint8_t *src, const zscrc_zs_record &r, uint64_t rel)
{
    const zspack::Piece pc = zspack::piece_at(r, rel);
    return pc.n ? zspack::gather8(src + pc.src_off, pc.n) : pc.word;
}
/* Whether the 8-byte word at p (a file offset minus ORIGIN) is record r's,
 * which starts at `start`, the last start at or before p if there is one. */
template <bool GAPS>
ZSREC_HD inline bool half_in_rec(const zscrc_zs_record &r, uint64_t start, uint64_t p, uint64_t *rel)
{
    if (GAPS)
        return zslog::word_in_rec(r, start, p, rel);
    *rel = p - start;
    return true;
}

/* The 16-byte word at file offset f (16-byte aligned, f + 16 > base, f < hi)
 * of the tile that ends at hi: its two halves and whether each is this sweep's
 * to write: not one before base, at or past hi or, with GAPS, in a commit
 * record.  recs: the records from the tile's first one on; s[0..m]: their
 * starts below hi - ORIGIN and the first one at or past it.  One search a word:
 * the second half lies in the same record or at the start of the next one. */
struct Word { uint64_t v0, v1; bool h0, h1; };
template <uint64_t ORIGIN, bool GAPS, class Starts>
ZSREC_HD inline Word word_at(const uint8_t *src, const zscrc_zs_record *recs, const Starts &s, uint64_t m, uint64_t f,
                             uint64_t base, uint64_t hi)
{
    const bool in0 = f >= base, in1 = f + 8 < hi;
    const uint64_t p = (in0 ? f : f + 8) - ORIGIN;
    uint64_t j = find_rec(s, m, p);
    zscrc_zs_record r = recs[j];
    Word w{0, 0, false, false};
    uint64_t rel;
    if (in0) {
        w.h0 = half_in_rec<GAPS>(r, s[j], p, &rel);
        if (w.h0)
            w.v0 = record_word(src, r, rel);
        if (in1 && p + 8 >= s[j + 1])
            r = recs[++j];
    }
    if (in1) {
        w.h1 = half_in_rec<GAPS>(r, s[j], f + 8 - ORIGIN, &rel);
        if (w.h1)
            w.v1 = record_word(src, r, rel);
    }
    return w;
}

/* How far the first record moves behind a tile of m staged starts that ends at
 * hi, s_m = s[m]: the next tile starts in record m - 1, or at record m's first
 * byte.  With GAPS a tile may lie before the first record (commits of empty
 * transactions come first): m = 0, and the first record stays.  Without GAPS
 * m >= 1: the tile's first record starts at or before its first byte. */
template <uint64_t ORIGIN, bool GAPS>
ZSREC_HD inline uint64_t advance(uint64_t s_m, uint64_t m, uint64_t hi)
{
    return s_m == hi - ORIGIN ? m : GAPS && m == 0 ? 0 : m - 1;
}

#ifdef __HIPCC__
static_assert(COPY_WG == zsdev::WG, "the copies run in the stages' workgroups");

/* The sweep of workgroup blockIdx.x of gridDim.x, all its threads calling: the
 * records of the list (recs, start[0..n] with start[n] = stop - ORIGIN) in
 * [base, stop), base < stop, into out.  s_start: LDS_STARTS words of LDS.
 * Every barrier is in workgroup-uniform control flow: the return of an empty
 * run depends on blockIdx only, the staging's break on the count all lanes got. */
template <uint64_t ORIGIN, bool GAPS>
__device__ inline void copy_tiles(const uint8_t *src, const zscrc_zs_record *recs, const uint64_t *start, uint64_t n,
                                  uint8_t *out, uint64_t T, uint64_t base, uint64_t stop, uint64_t *s_start)
{
    const Run run = run_of(blockIdx.x, gridDim.x, T, base, stop);
    if (run.t0 >= run.t1)
        return;
    /* the last record that starts at or before the run's first byte, or record 0 */
    uint64_t rec0 = find_rec(start, n, tile_lo(run.t0, T, base) - ORIGIN);
    for (uint64_t t = run.t0; t < run.t1; ++t) {
        const uint64_t hi = tile_hi(t, T, stop);
        /* s_start[j] = start[rec0 + j] up to the first one at or past hi (start[n] is) */
        uint32_t m = 0;
        for (uint32_t k = 0; k < LDS_STARTS; k += COPY_WG) {
            const uint64_t idx = rec0 + k + threadIdx.x;
            const uint64_t s = start[idx < n ? idx : n];
            s_start[k + threadIdx.x] = s;
            const uint32_t c = (uint32_t)__syncthreads_count(s < hi - ORIGIN);
            m += c;
            if (c < COPY_WG)
                break;
        }
        /* the 16-byte words of the tile: both halves as one store, or the one that is the sweep's */
        for (uint64_t w = threadIdx.x; w < T / 16; w += COPY_WG) {
            const uint64_t f = t * T + 16 * w;
            if (f + 16 <= base)
                continue;
            if (f >= hi)
                break;
            const Word v = word_at<ORIGIN, GAPS>(src, recs + rec0, s_start, m, f, base, hi);
            /* vmcnt(0).  Every load of this word has come back, but on a path the compiler cannot
             * rule out (neither half inside) the record's is still out; with its wait said here,
             * none comes to stand behind the stores, where it would wait for them too before the
             * next word's search (40 us of the packer's 810) */
            __builtin_amdgcn_s_waitcnt(0x0F70);
            if (v.h0 && v.h1) {
                *reinterpret_cast<zsdev::u64x2 *>(out + f) = zsdev::u64x2{v.v0, v.v1};
            } else if (v.h0) {
                *reinterpret_cast<uint64_t *>(out + f) = v.v0;
            } else if (!GAPS || v.h1) { /* without GAPS one half is inside, and written */
                *reinterpret_cast<uint64_t *>(out + f + 8) = v.v1;
            }
        }
        const uint64_t step = advance<ORIGIN, GAPS>(s_start[m], m, hi);
        __syncthreads(); /* s_start is rewritten by the next tile */
        rec0 += step;
    }
}
#endif /* __HIPCC__ */

} /* namespace zstile */

#endif
