/*
 * log_layout.cpp -- the device log writer's layout arithmetic on the CPU
 * (tests/test_log_layout.py).  Includes only the headers the kernels of
 * zscrc_devlog.hip share with the host, reads a case file
 *
 *   u64 src_len, n, n_tx (2^64-1: no table, one transaction a record), at,
 *       finalise, prev_crc, file_len, shift, startidx, endidx; uuid[16];
 *   src[src_len]; recs[n] (4 x u64); tx_end[n_tx]; file[file_len] (the expected
 *   image, its first `at` bytes the image appended to)
 *
 * and rebuilds the image the way the kernels do: lengths and delete marks to
 * P[] and D[], the table checked, the spans and C[], the totals, the starts,
 * then for each tile size the records tile by tile in file coordinates and
 * word by word (find_rec, word_in_rec, piece_at, gather8), the commit records
 * from the span CRCs, the finalise commit, the header.  The source lies at an
 * address = shift mod 8 in an allocation that ends with its last 8-byte
 * granule, so a sanitizer sees any read outside the aligned words that hold
 * source bytes.  Exit status 0 = every byte equal at every tile size.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../zeroskip_amd/csrc/zscrc_log_layout.h"

using namespace zspack;
using namespace zslog;

static int fail(const char *what, uint64_t a, uint64_t b, uint64_t c)
{
    fprintf(stderr, "log_layout: %s (%llu, %llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b,
            (unsigned long long)c);
    return 1;
}

static uint32_t g_tab[256];
static uint32_t crc_span(const uint8_t *p, uint64_t n)
{
    if (!g_tab[1])
        for (uint32_t b = 0; b < 256; ++b)
            g_tab[b] = ~crc_bytes(~0u, b, 1); /* the register step of one byte from 0 */
    uint32_t c = ~0u;
    for (uint64_t i = 0; i < n; ++i)
        c = g_tab[(c ^ p[i]) & 0xFF] ^ (c >> 8);
    return ~c;
}

int main(int argc, char **argv)
{
    if (argc != 2)
        return fail("usage: log_layout CASEFILE", 0, 0, 0);
    FILE *f = fopen(argv[1], "rb");
    uint64_t hd[10];
    uint8_t uuid[16];
    if (!f || fread(hd, 8, 10, f) != 10 || fread(uuid, 1, 16, f) != 16)
        return fail("cannot read the case", 0, 0, 0);
    const uint64_t src_len = hd[0], n = hd[1], at = hd[3], file_len = hd[6], shift = hd[7] & 7;
    const bool table = hd[2] != U64_MAX, finalise = hd[4] != 0;
    const uint64_t ntx = table ? hd[2] : n;
    const uint64_t gran = (shift + src_len + 7) & ~7ull;
    uint8_t *buf = static_cast<uint8_t *>(malloc(gran ? gran : 8));
    uint8_t *src = buf + shift;
    std::vector<zscrc_zs_record> recs(n);
    std::vector<uint64_t> ends(table ? ntx + 1 : 1); /* never NULL: an empty table is a table */
    std::vector<uint8_t> want(file_len);
    if ((src_len && fread(src, 1, src_len, f) != src_len) || (n && fread(recs.data(), 32, n, f) != n) ||
        (table && ntx && fread(ends.data(), 8, ntx, f) != ntx) ||
        (file_len && fread(want.data(), 1, file_len, f) != file_len))
        return fail("short case file", src_len, n, file_len);
    fclose(f);
    const uint64_t *tx_end = table ? ends.data() : nullptr;
    if (!at_ok(at) || at > file_len)
        return fail("position", at, file_len, 0);

    /* P[], D[] */
    std::vector<uint64_t> P(n + 1), D(n), C(ntx + 1), first(ntx), slen(ntx), start(n + 1);
    uint64_t top = 0;
    P[0] = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (rec_bad(recs[i], src_len))
            return fail("bad record", i, recs[i].key_off, recs[i].key_len);
        P[i + 1] = sat_add(P[i], rec_len(recs[i]));
        top = mark_max(top, del_mark(recs[i], i));
        D[i] = top;
    }
    /* the table, the spans, C[] */
    if (table && !ntx && n)
        return fail("records without a transaction", n, 0, 0);
    C[0] = 0;
    for (uint64_t t = 0; t < ntx; ++t) {
        const uint64_t b = tx_begin(tx_end, t), e = tx_stop(tx_end, t);
        if (!tx_ok(b, e, t, ntx, n))
            return fail("bad table entry", t, b, e);
        const uint64_t s = span_first(b, e, e > b ? D[e - 1] : 0);
        if (s < b || (e > b && s >= e) || (e == b && s != b))
            return fail("span start outside its transaction", t, s, e);
        for (uint64_t i = s + 1; i < e; ++i)
            if (is_delete(recs[i]))
                return fail("a delete behind the span start", t, s, i);
        if (s > b && !is_delete(recs[s]))
            return fail("span starts at an add that is not the first record", t, s, b);
        first[t] = P[s];
        slen[t] = span_bytes(P[s], P[e]);
        C[t + 1] = C[t] + commit_len(slen[t]);
    }
    const Totals tot = totals(at, P[n], C[ntx], ntx, finalise);
    if (tot.end != file_len)
        return fail("end offset", tot.end, file_len, P[n]);
    const uint64_t base = base_of(at);
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t t = tx_of(tx_end, ntx, i);
        if (t >= ntx || tx_begin(tx_end, t) > i || tx_stop(tx_end, t) <= i)
            return fail("transaction of a record", i, t, ntx);
        start[i] = placed(base, P[i], C[t]);
    }
    start[n] = tot.body_end;

    const uint64_t tiles[4] = {64, 128, 4096, 65536};
    for (uint64_t T : tiles) {
        /* 8-byte words, so that the output is built the way the kernel stores it */
        std::vector<uint64_t> out(file_len / 8 + 1, 0xA5A5A5A5A5A5A5A5ull);
        memcpy(out.data(), want.data(), at);
        uint64_t written = 0;
        if (n) {
            const uint64_t stop = tot.body_end, tlo = base / T, thi = (stop + T - 1) / T;
            uint64_t rec0 = find_rec(start, n, base);
            for (uint64_t t = tlo; t < thi; ++t) {
                const uint64_t f0 = t * T, lo = f0 > base ? f0 : base, hi = f0 + T < stop ? f0 + T : stop;
                if (lo >= hi)
                    return fail("tile range", t, lo, hi);
                if (rec0 != find_rec(start, n, lo))
                    return fail("running first record", t, rec0, find_rec(start, n, lo));
                const uint64_t *s = start.data() + rec0;
                uint64_t m = 0;
                while (s[m] < hi)
                    ++m;
                if (m > T / 24 + 2 || (m == 0 && rec0 != 0))
                    return fail("records of a tile", t, m, T);
                for (uint64_t p = lo; p < hi; p += 8) {
                    const uint64_t j = find_rec(s, m, p);
                    uint64_t rel;
                    if (!word_in_rec(recs[rec0 + j], s[j], p, &rel))
                        continue; /* a commit record's word */
                    const Piece pc = piece_at(recs[rec0 + j], rel);
                    out[p / 8] = pc.n ? gather8(src + pc.src_off, pc.n) : pc.word;
                    ++written;
                }
                rec0 += s[m] == hi ? m : m ? m - 1 : 0;
            }
        }
        if (written != P[n] / 8)
            return fail("words written", written, P[n] / 8, T);
        /* commits, the finalise commit, header */
        const uint8_t *ob = reinterpret_cast<const uint8_t *>(out.data());
        uint64_t w[3];
        uint32_t stored, reg = (uint32_t)hd[5];
        for (uint64_t t = 0; t < ntx; ++t) {
            const uint64_t off = placed(base, first[t], C[t]);
            reg = crc_span(ob + off, slen[t]);
            const int k = commit_words(reg, slen[t], false, w, &stored);
            if ((uint64_t)k * 8 != commit_len(slen[t]) || out[(off + slen[t]) / 8] != 0xA5A5A5A5A5A5A5A5ull)
                return fail("commit record", t, off, slen[t]);
            for (int i = 0; i < k; ++i)
                out[(off + slen[t]) / 8 + i] = w[i];
        }
        if (finalise) {
            commit_words(reg, 0, false, w, &stored);
            out[tot.body_end / 8] = w[0];
        }
        if (at == 0) {
            const Header h = header_words(uuid, (uint32_t)hd[8], (uint32_t)hd[9]);
            for (int i = 0; i < 5; ++i)
                out[i] = h.w[i];
        }
        if (memcmp(ob, want.data(), file_len) != 0) {
            uint64_t d = 0;
            while (ob[d] == want[d])
                ++d;
            return fail("byte differs at, tile, file", d, T, file_len);
        }
        if (out[file_len / 8] != 0xA5A5A5A5A5A5A5A5ull)
            return fail("word past the end written", T, file_len, 0);
    }
    free(buf);
    printf("ok %llu records %llu commits %llu bytes\n", (unsigned long long)n, (unsigned long long)tot.commits,
           (unsigned long long)file_len);
    return 0;
}
