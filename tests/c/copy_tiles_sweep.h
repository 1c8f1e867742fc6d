/*
 * copy_tiles_sweep.h -- what pack_layout.cpp and log_layout.cpp share: the
 * tile sweep of pack_copy_kernel and log_copy_kernel on the CPU.  The run of
 * tiles of a workgroup, the 16-byte word and the advance of the first record
 * are zscrc_copy_tiles.h's functions, the ones the kernels call; workgroups
 * and lanes are played by loops, the staged starts by the list itself, and the
 * halves are stored the way the kernel stores them.  PROGRAM names the program.
 */
#include <cstdio>
#include <vector>

#include "../../zeroskip_amd/csrc/zscrc_copy_tiles.h"

static const uint64_t CANARY = 0xA5A5A5A5A5A5A5A5ull;

static int fail(const char *what, uint64_t a, uint64_t b, uint64_t c)
{
    fprintf(stderr, "%s: %s (%llu, %llu, %llu)\n", PROGRAM, what, (unsigned long long)a, (unsigned long long)b,
            (unsigned long long)c);
    return 1;
}

static uint32_t crc_span(const uint8_t *p, uint64_t n)
{
    static uint32_t tab[256];
    if (!tab[1])
        for (uint32_t b = 0; b < 256; ++b)
            tab[b] = ~zspack::crc_bytes(~0u, b, 1); /* the register step of one byte from 0 */
    uint32_t c = ~0u;
    for (uint64_t i = 0; i < n; ++i)
        c = tab[(c ^ p[i]) & 0xFF] ^ (c >> 8);
    return ~c;
}

/* stores of 16 bytes, of a first half and of a second half */
struct Stores { uint64_t both, first, second; };

/* The records of [base, stop) into out (8-byte words by file offset, canaries
 * behind the bytes the call keeps) at tile T, by grids of 1, 2, 7 and one
 * workgroup more than there are tiles, so that some runs are empty: the runs
 * partition the tiles, every grid writes want_words words and the same bytes. */
template <uint64_t ORIGIN, bool GAPS>
static int sweep(const uint8_t *src, const std::vector<zscrc_zs_record> &recs, const std::vector<uint64_t> &start,
                 uint64_t T, uint64_t base, uint64_t stop, uint64_t want_words, std::vector<uint64_t> &out, Stores &st)
{
    using namespace zstile;
    const uint64_t n = recs.size(), tlo = base / T, thi = (stop + T - 1) / T, grids[4] = {1, 2, 7, thi - tlo + 1};
    const std::vector<uint64_t> blank = out;
    for (uint64_t g : grids) {
        std::vector<uint64_t> cur = blank;
        uint64_t next = tlo, words = 0;
        for (uint64_t b = 0; b < g; ++b) {
            const Run run = run_of(b, g, T, base, stop);
            if (run.t0 >= run.t1)
                continue;
            if (run.t0 != next || run.t1 > thi)
                return fail("a run's tiles twice, left out or past the end", b, run.t0, next);
            next = run.t1;
            uint64_t rec0 = find_rec(start, n, tile_lo(run.t0, T, base) - ORIGIN);
            for (uint64_t t = run.t0; t < run.t1; ++t) {
                const uint64_t lo = tile_lo(t, T, base), hi = tile_hi(t, T, stop);
                if (lo >= hi || hi > stop || (t + 1 == thi) != (hi == stop))
                    return fail("tile range", t, lo, hi);
                if (rec0 != find_rec(start, n, lo - ORIGIN))
                    return fail("running first record", t, rec0, find_rec(start, n, lo - ORIGIN));
                const uint64_t *s = start.data() + rec0;
                uint64_t m = 0;
                while (s[m] < hi - ORIGIN)
                    ++m;
                if (m > T / 24 + 2 || (m == 0 && (!GAPS || rec0 != 0)))
                    return fail("records of a tile", t, m, T);
                for (uint64_t f = t * T; f < hi; f += 16) {
                    if (f + 16 <= base)
                        continue;
                    const Word v = word_at<ORIGIN, GAPS>(src, recs.data() + rec0, s, m, f, base, hi);
                    if ((v.h0 && f < lo) || (v.h1 && f + 8 >= hi))
                        return fail("half outside its tile", t, f, T);
                    if (v.h0)
                        cur[f / 8] = v.v0;
                    if (v.h1)
                        cur[f / 8 + 1] = v.v1;
                    words += v.h0 + v.h1;
                    st.both += v.h0 && v.h1; /* the kernel's three stores */
                    st.first += v.h0 && !v.h1;
                    st.second += v.h1 && !v.h0;
                }
                rec0 += advance<ORIGIN, GAPS>(s[m], m, hi);
            }
        }
        if (next != thi)
            return fail("tiles left out", next, thi, g);
        if (words != want_words)
            return fail("words written", words, want_words, T);
        if (g != 1 && cur != out)
            return fail("bytes differ between grid sizes", T, g, 0);
        out.swap(cur);
    }
    return 0;
}
