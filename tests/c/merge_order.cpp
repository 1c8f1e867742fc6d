/*
 * merge_order.cpp -- the device merge's order arithmetic on the CPU
 * (tests/test_merge_order.py).  Includes only the header the kernels of
 * zscrc_merge.hip share with the host, reads a case file
 *
 *   u64 src_len, k, n_total, n_want, shift, drop_deletes;
 *   k x (u64 n, base); src[src_len]; recs[n_total] (4 x u64, not rebased);
 *   want[n_want] (4 x u64: the winners in key order, rebased)
 *
 * and merges the way the kernels do, at tiles of 64 and 256 entries: every
 * record rebased and checked, its sort entry, each tile through the bitonic
 * network with the keys' second words beside the entries, then the passes --
 * an output tile's cut of two runs by two diagonal searches, its pieces staged,
 * each thread's cut by a search among them and its few entries merged -- and
 * the winner rule.  The source lies at an address = shift mod 8 in an
 * allocation that ends with its last 8-byte granule, so a sanitizer sees any
 * read outside the aligned words that hold source bytes.
 * Exit status 0 = the winners equal the expected list at both tile sizes.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../zeroskip_amd/csrc/zscrc_merge_order.h"

using namespace zsmerge;

static int fail(const char *what, uint64_t a, uint64_t b, uint64_t c)
{
    fprintf(stderr, "merge_order: %s (%llu, %llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b,
            (unsigned long long)c);
    return 1;
}

struct KeyLess {
    Keys K;
    bool operator()(const Entry &a, const Entry &b) const { return less(K, a, b); }
};

int main(int argc, char **argv)
{
    if (argc != 2)
        return fail("usage: merge_order CASEFILE", 0, 0, 0);
    FILE *f = fopen(argv[1], "rb");
    uint64_t hd[6];
    if (!f || fread(hd, 8, 6, f) != 6)
        return fail("cannot read the case", 0, 0, 0);
    const uint64_t src_len = hd[0], k = hd[1], n = hd[2], n_want = hd[3], shift = hd[4] & 7;
    const bool drop = hd[5] != 0;
    std::vector<uint64_t> lists(2 * k);
    const uint64_t gran = (shift + src_len + 7) & ~7ull;
    uint8_t *buf = static_cast<uint8_t *>(malloc(gran ? gran : 8));
    uint8_t *src = buf + shift;
    std::vector<zscrc_zs_record> recs(n), want(n_want);
    if ((k && fread(lists.data(), 16, k, f) != k) || (src_len && fread(src, 1, src_len, f) != src_len) ||
        (n && fread(recs.data(), 32, n, f) != n) || (n_want && fread(want.data(), 32, n_want, f) != n_want))
        return fail("short case file", src_len, n, n_want);
    fclose(f);

    /* the gather: rebase, check, entry */
    std::vector<Entry> first(n);
    uint64_t seq = 0;
    for (uint64_t l = 0; l < k; ++l)
        for (uint64_t j = 0; j < lists[2 * l]; ++j, ++seq) {
            if (seq >= n)
                return fail("more records in the lists than n_total", l, j, n);
            if (!rebase(recs[seq], lists[2 * l + 1], src_len))
                return fail("record outside the source", seq, recs[seq].key_off, recs[seq].key_len);
            first[seq] = make_entry(src, recs[seq], (uint32_t)seq);
        }
    if (seq != n)
        return fail("fewer records in the lists than n_total", seq, n, 0);
    const Keys K{src, recs.data()};
    const KeyLess lt{K};

    const uint32_t tiles[2] = {64, 256}, WG = 256;
    for (uint32_t T : tiles) {
        std::vector<Entry> e0(first), e1(n);
        /* the tile sort */
        for (uint64_t t0 = 0; t0 < n; t0 += T) {
            std::vector<Entry> s(T, Entry{0, SEQ_PAD, 0});
            std::vector<uint64_t> w(T, 0);
            for (uint32_t i = 0; i < T && t0 + i < n; ++i) {
                s[i] = e0[t0 + i];
                if (s[i].len > 8)
                    w[i] = key_word(src, recs[s[i].seq].key_off, recs[s[i].seq].key_len, 8);
            }
            for (uint32_t kk = 2; kk <= T; kk <<= 1)
                for (uint32_t j = kk >> 1; j > 0; j >>= 1)
                    for (uint32_t t = 0; t < T / 2; ++t) {
                        uint32_t lo;
                        bool up;
                        bitonic_pair(t, kk, j, &lo, &up);
                        if (lo + j >= T)
                            return fail("bitonic pair outside the tile", t, kk, j);
                        if (less_tile(K, s[lo + j], w[lo + j], s[lo], w[lo]) == up) {
                            std::swap(s[lo], s[lo + j]);
                            std::swap(w[lo], w[lo + j]);
                        }
                    }
            for (uint32_t i = 0; i < T && t0 + i < n; ++i) {
                if (s[i].seq == SEQ_PAD)
                    return fail("padding sorted before a record", t0, i, T);
                e0[t0 + i] = s[i];
            }
        }
        /* the passes */
        Entry *in = e0.data(), *out = e1.data();
        for (uint64_t run = T; run < n; run *= 2) {
            for (uint64_t o0 = 0; o0 < n; o0 += T) {
                const uint32_t cnt = n - o0 < T ? (uint32_t)(n - o0) : T;
                const uint64_t a0 = o0 / (2 * run) * (2 * run);
                const uint32_t na = n - a0 < run ? (uint32_t)(n - a0) : (uint32_t)run;
                const uint64_t b0 = a0 + na;
                const uint32_t nb = n - b0 < run ? (uint32_t)(n - b0) : (uint32_t)run;
                if (nb == 0) {
                    for (uint32_t i = 0; i < cnt; ++i)
                        out[o0 + i] = in[o0 + i];
                    continue;
                }
                const uint32_t d0 = (uint32_t)(o0 - a0);
                const Entry *ra = in + a0, *rb = in + b0;
                const uint32_t i0 = diag_search(ra, na, rb, nb, d0, lt), i1 = diag_search(ra, na, rb, nb, d0 + cnt, lt);
                if (i1 < i0 || i1 - i0 > cnt || d0 - i0 > nb)
                    return fail("cuts of a tile", o0, i0, i1);
                const uint32_t ca = i1 - i0, cb = cnt - ca;
                std::vector<Entry> s(cnt);
                for (uint32_t i = 0; i < cnt; ++i)
                    s[i] = i < ca ? ra[i0 + i] : rb[d0 - i0 + (i - ca)];
                const uint32_t vt = (T + WG - 1) / WG;
                const Entry *sa = s.data(), *sb = s.data() + ca;
                for (uint32_t d = 0; d < cnt; d += vt) {
                    uint32_t i = diag_search(sa, ca, sb, cb, d, lt), j = d - i;
                    for (uint32_t v = 0; v < vt && d + v < cnt; ++v) {
                        const bool take_a = j >= cb || (i < ca && !lt(sb[j], sa[i]));
                        out[o0 + d + v] = take_a ? sa[i++] : sb[j++];
                    }
                }
            }
            std::swap(in, out);
        }
        /* sorted by (key, seq), every record once */
        std::vector<uint8_t> seen(n, 0);
        for (uint64_t i = 0; i < n; ++i) {
            if (in[i].seq >= n || seen[in[i].seq]++)
                return fail("not a permutation at", i, in[i].seq, T);
            if (i && !less(K, in[i - 1], in[i]))
                return fail("not ascending at", i, in[i - 1].seq, in[i].seq);
        }
        /* the winners */
        uint64_t m = 0;
        for (uint64_t i = 0; i < n; ++i) {
            if (winner_flag(K, in, i, n, drop) != F_WINNER)
                continue;
            if (m >= n_want || memcmp(&recs[in[i].seq], &want[m], 32) != 0)
                return fail("winner differs at, seq, tile", m, in[i].seq, T);
            ++m;
        }
        if (m != n_want)
            return fail("winners", m, n_want, T);
    }
    free(buf);
    printf("ok %llu records %llu winners\n", (unsigned long long)n, (unsigned long long)n_want);
    return 0;
}
