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
 * then for each tile size the records by the kernel's own tile sweep
 * (copy_tiles_sweep.h) at four grid sizes, the commit records from the span
 * CRCs, the finalise commit, the header.  The source lies at an address =
 * shift mod 8 in an allocation that ends with its last 8-byte granule, so a
 * sanitizer sees any read outside the aligned words that hold source bytes.
 * Exit status 0 = every byte equal at every tile and grid size; the ok line
 * counts the stores of each kind.
 */
#include <cstdlib>
#include <cstring>

static const char *PROGRAM = "log_layout";
#include "copy_tiles_sweep.h"

using namespace zspack;
using namespace zslog;

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
    Stores stores{0, 0, 0};
    for (uint64_t T : tiles) {
        /* 8-byte words, so that the output is built the way the kernel stores it */
        std::vector<uint64_t> out(file_len / 8 + 1, CANARY);
        memcpy(out.data(), want.data(), at);
        if (n && sweep<0, true>(src, recs, start, T, base, tot.body_end, P[n] / 8, out, stores))
            return 1;
        /* commits, the finalise commit, header */
        const uint8_t *ob = reinterpret_cast<const uint8_t *>(out.data());
        uint64_t w[3];
        uint32_t stored, reg = (uint32_t)hd[5];
        for (uint64_t t = 0; t < ntx; ++t) {
            const uint64_t off = placed(base, first[t], C[t]);
            reg = crc_span(ob + off, slen[t]);
            const int k = commit_words(reg, slen[t], false, w, &stored);
            if ((uint64_t)k * 8 != commit_len(slen[t]) || out[(off + slen[t]) / 8] != CANARY)
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
        if (out[file_len / 8] != CANARY)
            return fail("word past the end written", T, file_len, 0);
    }
    free(buf);
    printf("ok %llu records %llu commits %llu bytes; stores: %llu of 16 bytes, %llu of a first half, %llu of a second half\n",
           (unsigned long long)n, (unsigned long long)tot.commits, (unsigned long long)file_len,
           (unsigned long long)stores.both, (unsigned long long)stores.first, (unsigned long long)stores.second);
    return 0;
}
