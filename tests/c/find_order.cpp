/*
 * find_order.cpp -- the device lookup's search arithmetic on the CPU
 * (tests/test_find_order.py).  Includes only the header the kernels of
 * zscrc_find.hip share with the host, reads a case file
 *
 *   u64 src_len, k, n_total, qsrc_len, nq, shift, qshift;
 *   k x (u64 n, base); src[src_len]; recs[n_total] (4 x u64, not rebased);
 *   qsrc[qsrc_len]; queries[nq] (4 x u64); want[nq] (4 x u64: the hits)
 *
 * and searches the way the kernels do, at 1, 2, 64 and 2,048 splitters: every
 * record rebased and checked, its key against its predecessor's in its level,
 * every level's table from the splitter positions, a copy of the table (the
 * kernels' LDS), then the levels in order -- the bucket from the table, the
 * bisection inside it -- and the hit.  The bucket must hold the lower bound
 * that the plain bisection finds.  The source and the query bytes lie at
 * addresses = shift and qshift mod 8 in allocations that end with their last
 * 8-byte granule, so a sanitizer sees any read outside the aligned words that
 * hold their bytes.
 * Exit status 0 = the hits equal the expected ones at every table size.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../zeroskip_amd/csrc/zscrc_find_order.h"

using namespace zsfind;

static int fail(const char *what, uint64_t a, uint64_t b, uint64_t c)
{
    fprintf(stderr, "find_order: %s (%llu, %llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b,
            (unsigned long long)c);
    return 1;
}

static uint8_t *granules(uint64_t shift, uint64_t len)
{
    const uint64_t gran = (shift + len + 7) & ~7ull;
    return static_cast<uint8_t *>(malloc(gran ? gran : 8));
}

int main(int argc, char **argv)
{
    if (argc != 2)
        return fail("usage: find_order CASEFILE", 0, 0, 0);
    FILE *f = fopen(argv[1], "rb");
    uint64_t hd[7];
    if (!f || fread(hd, 8, 7, f) != 7)
        return fail("cannot read the case", 0, 0, 0);
    const uint64_t src_len = hd[0], k = hd[1], n = hd[2], qsrc_len = hd[3], nq = hd[4], shift = hd[5] & 7,
                   qshift = hd[6] & 7;
    std::vector<uint64_t> lists(2 * k);
    uint8_t *buf = granules(shift, src_len), *qbuf = granules(qshift, qsrc_len);
    uint8_t *src = buf + shift, *qsrc = qbuf + qshift;
    std::vector<zscrc_zs_record> recs(n), queries(nq);
    std::vector<Hit> want(nq);
    if (k && fread(lists.data(), 16, k, f) != k)
        return fail("short case file: lists", k, 0, 0);
    if ((src_len && fread(src, 1, src_len, f) != src_len) || (n && fread(recs.data(), 32, n, f) != n))
        return fail("short case file: source and records", src_len, n, 0);
    if ((qsrc_len && fread(qsrc, 1, qsrc_len, f) != qsrc_len) || (nq && fread(queries.data(), 32, nq, f) != nq) ||
        (nq && fread(want.data(), 32, nq, f) != nq))
        return fail("short case file: queries", qsrc_len, nq, 0);
    fclose(f);

    /* the check: bounds, then the order inside a level */
    std::vector<Level> levels(k);
    uint64_t seq = 0;
    for (uint64_t l = 0; l < k; ++l) {
        levels[l] = Level{recs.data() + seq, lists[2 * l], lists[2 * l + 1]};
        if (lists[2 * l] > n - seq)
            return fail("more records in the lists than n_total", l, seq, n);
        for (uint64_t j = 0; j < levels[l].n; ++j, ++seq) {
            zscrc_zs_record r = recs[seq];
            if (!zsmerge::rebase(r, levels[l].base, src_len))
                return fail("record outside the source", seq, r.key_off, r.key_len);
            if (j == 0)
                continue;
            zscrc_zs_record prev = recs[seq - 1];
            zsmerge::rebase(prev, levels[l].base, src_len);
            if (order_offence(src, prev, r))
                return fail("a level does not ascend at", seq, l, j);
        }
    }
    if (seq != n)
        return fail("fewer records in the lists than n_total", seq, n, 0);

    const uint32_t sizes[4] = {1, 2, 64, 2048};
    for (uint32_t S : sizes) {
        /* the tables, and the copy a workgroup searches */
        std::vector<std::vector<uint64_t>> tabs(k);
        for (uint64_t l = 0; l < k && S > 1; ++l) {
            if (!levels[l].n)
                continue;
            std::vector<uint64_t> t(4 * (size_t)S);
            uint64_t before = 0;
            for (uint32_t j = 0; j < S; ++j) {
                const uint64_t at = splitter_pos(j, levels[l].n, S);
                if (at >= levels[l].n || at < before || (j == 0 && at != 0))
                    return fail("splitter position", j, at, levels[l].n);
                before = at;
                const zscrc_zs_record &r = levels[l].recs[at];
                table_store(t.data(), S, j, src, r.key_off + levels[l].base, r.key_len);
            }
            tabs[l] = t;
        }
        for (uint64_t i = 0; i < nq; ++i) {
            Hit h{NONE, 0, 0, 0};
            if (!key_ok(queries[i].key_off, queries[i].key_len, qsrc_len)) {
                h.level = BAD_QUERY;
            } else {
                const Query q = make_query(qsrc, queries[i].key_off, queries[i].key_len);
                for (uint64_t l = 0; l < k && h.level == NONE; ++l) {
                    bool found, plain_found;
                    const uint64_t at = find_in_level(qsrc, q, src, levels[l], tabs[l].data(), S, &found);
                    const uint64_t plain = find_in_level(qsrc, q, src, levels[l], nullptr, 1, &plain_found);
                    if (at != plain || found != plain_found)
                        return fail("the bucket search and the plain bisection differ: query, level, S", i, l, S);
                    if (at > levels[l].n)
                        return fail("lower bound outside the level", i, at, levels[l].n);
                    if (found)
                        h = hit_of(levels[l], l, at);
                    else
                        h.location = l + 1 == k ? at : 0;
                }
            }
            if (memcmp(&h, &want[i], 32) != 0)
                return fail("hit differs at query, S, level found", i, S, h.level);
        }
    }
    free(buf);
    free(qbuf);
    printf("ok %llu records %llu queries\n", (unsigned long long)n, (unsigned long long)nq);
    return 0;
}
