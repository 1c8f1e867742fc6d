/*
 * scan_order.cpp -- the device prefix scan's arithmetic on the CPU
 * (tests/test_scan_order.py).  Includes only the header the kernels of
 * zscrc_scan.hip share with the host, reads a case file
 *
 *   u64 src_len, k, n_total, qsrc_len, nq, shift, qshift, keep_deletes, m;
 *   k x (u64 n, base); src[src_len]; recs[n_total] (4 x u64, not rebased);
 *   qsrc[qsrc_len]; queries[nq] (4 x u64); offs[nq + 1]; rows[m] (4 x u64);
 *   seqs[m]                  (m = 2^64 - 1: nothing to compare, no offs / rows /
 *                             seqs follow and the levels need not ascend)
 *
 * and scans the way the kernels do, at 1, 2, 64, 1,024 (the default) and
 * 2,048 splitters: every record rebased and checked, every level's table, a copy of it (the kernels'
 * LDS), the bounds of every (query, level) pair through the table -- which must
 * equal the bounds without one -- the scan of the range lengths, every
 * candidate decomposed and ranked into its slot behind the guard, the winners
 * compacted in slot order.  Every position is checked against its array before
 * it is used, and the arrays are exact allocations, so a sanitizer sees what
 * the checks miss.  For ascending levels every slot must be written exactly
 * once.  The source and the query bytes lie at addresses = shift and qshift
 * mod 8 in allocations that end with their last 8-byte granule.
 * Exit status 0 = rows, offsets and seqs equal the expected ones at every
 * table size.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../zeroskip_amd/csrc/zscrc_scan_order.h"

using namespace zsfind;
using namespace zsscan;

static int fail(const char *what, uint64_t a, uint64_t b, uint64_t c)
{
    fprintf(stderr, "scan_order: %s (%llu, %llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b,
            (unsigned long long)c);
    return 1;
}

static uint8_t *granules(uint64_t shift, uint64_t len)
{
    const uint64_t gran = (shift + len + 7) & ~7ull;
    return static_cast<uint8_t *>(malloc(gran ? gran : 8));
}

template <class T>
static T *exact(uint64_t n)
{
    return static_cast<T *>(malloc(n ? n * sizeof(T) : 1));
}

int main(int argc, char **argv)
{
    if (argc != 2)
        return fail("usage: scan_order CASEFILE", 0, 0, 0);
    FILE *f = fopen(argv[1], "rb");
    uint64_t hd[9];
    if (!f || fread(hd, 8, 9, f) != 9)
        return fail("cannot read the case", 0, 0, 0);
    const uint64_t src_len = hd[0], k = hd[1], n = hd[2], qsrc_len = hd[3], nq = hd[4], shift = hd[5] & 7,
                   qshift = hd[6] & 7, m = hd[8];
    const bool keep = hd[7] != 0, compare = m != ~0ull;
    std::vector<uint64_t> lists(2 * k);
    uint8_t *buf = granules(shift, src_len), *qbuf = granules(qshift, qsrc_len);
    uint8_t *src = buf + shift, *qsrc = qbuf + qshift;
    std::vector<zscrc_zs_record> recs(n), queries(nq), want(compare ? m : 0);
    std::vector<uint64_t> want_offs(compare ? nq + 1 : 0), want_seq(compare ? m : 0);
    if (k && fread(lists.data(), 16, k, f) != k)
        return fail("short case file: lists", k, 0, 0);
    if ((src_len && fread(src, 1, src_len, f) != src_len) || (n && fread(recs.data(), 32, n, f) != n))
        return fail("short case file: source and records", src_len, n, 0);
    if ((qsrc_len && fread(qsrc, 1, qsrc_len, f) != qsrc_len) || (nq && fread(queries.data(), 32, nq, f) != nq))
        return fail("short case file: queries", qsrc_len, nq, 0);
    if (compare && (fread(want_offs.data(), 8, nq + 1, f) != nq + 1 || (m && fread(want.data(), 32, m, f) != m) ||
                    (m && fread(want_seq.data(), 8, m, f) != m)))
        return fail("short case file: expected rows", m, nq, 0);
    fclose(f);

    /* the check, and the levels that are not empty with the seq of their first record */
    std::vector<Level> levels;
    std::vector<uint64_t> firsts;
    uint64_t seq = 0;
    for (uint64_t l = 0; l < k; ++l) {
        const Level lv{recs.data() + seq, lists[2 * l], lists[2 * l + 1]};
        if (lv.n > n - seq)
            return fail("more records in the lists than n_total", l, seq, n);
        if (lv.n) {
            levels.push_back(lv);
            firsts.push_back(seq);
        }
        for (uint64_t j = 0; j < lv.n; ++j, ++seq) {
            zscrc_zs_record r = recs[seq];
            if (!zsmerge::rebase(r, lv.base, src_len))
                return fail("record outside the source", seq, r.key_off, r.key_len);
            if (j == 0 || !compare)
                continue;
            zscrc_zs_record prev = recs[seq - 1];
            zsmerge::rebase(prev, lv.base, src_len);
            if (order_offence(src, prev, r))
                return fail("a level does not ascend at", seq, l, j);
        }
    }
    if (seq != n)
        return fail("fewer records in the lists than n_total", seq, n, 0);
    const uint32_t F = (uint32_t)levels.size();
    const uint64_t pairs = nq * F;

    const uint32_t sizes[5] = {1, 2, 64, 1024, 2048}; /* 1,024: the default */
    for (uint32_t S : sizes) {
        /* the tables, and the copy a workgroup searches */
        std::vector<std::vector<uint64_t>> tabs(F);
        for (uint32_t l = 0; l < F && S > 1; ++l) {
            std::vector<uint64_t> t(4 * (size_t)S);
            for (uint32_t j = 0; j < S; ++j) {
                const zscrc_zs_record &r = levels[l].recs[splitter_pos(j, levels[l].n, S)];
                table_store(t.data(), S, j, src, r.key_off + levels[l].base, r.key_len);
            }
            tabs[l] = t;
        }
        /* the bounds: the matrix of lower bounds and range lengths, query major */
        uint32_t *lo = exact<uint32_t>(pairs);
        uint64_t *start = exact<uint64_t>(pairs + 1);
        for (uint64_t i = 0; i < nq; ++i) {
            const bool ok = key_ok(queries[i].key_off, queries[i].key_len, qsrc_len);
            const Query p = ok ? make_query(qsrc, queries[i].key_off, queries[i].key_len) : Query{};
            for (uint32_t l = 0; l < F; ++l) {
                uint64_t a = 0, b = 0;
                if (ok) {
                    bool found, plain_found;
                    a = find_in_level(qsrc, p, src, levels[l], tabs[l].data(), S, &found);
                    b = prefix_end(qsrc, p, src, levels[l], tabs[l].data(), S, a);
                    const uint64_t pa = find_in_level(qsrc, p, src, levels[l], nullptr, 1, &plain_found);
                    const uint64_t pb = prefix_end(qsrc, p, src, levels[l], nullptr, 1, pa);
                    if (compare && (a != pa || b != pb))
                        return fail("the bounds through the table and without differ: query, level, S", i, l, S);
                    if (a > b || b > levels[l].n)
                        return fail("bounds outside the level: query, lo, hi", i, a, b);
                }
                lo[i * F + l] = (uint32_t)a;
                start[i * F + l] = b - a;
            }
        }
        /* the scan of the lengths */
        uint64_t C = 0;
        for (uint64_t e = 0; e < pairs; ++e) {
            const uint64_t cnt = start[e];
            start[e] = C;
            C += cnt;
        }
        start[pairs] = C;
        /* the rank: every candidate into its slot */
        uint32_t *slots = exact<uint32_t>(C);
        for (uint64_t c = 0; c < C; ++c)
            slots[c] = SLOT_SUPERSEDED;
        std::vector<uint8_t> written(C, 0);
        for (uint64_t c = 0; c < C; ++c) {
            const Cand d = decompose(start, lo, pairs, F, c);
            if (d.pair >= pairs || d.query >= nq || d.level >= F || d.rec >= levels[d.level].n ||
                c < start[d.pair] || c >= start[d.pair + 1])
                return fail("decomposition outside its arrays: candidate, pair, record", c, d.pair, d.rec);
            const Level &lv = levels[d.level];
            const zscrc_zs_record rec = lv.recs[d.rec];
            const Query key = make_query(src, rec.key_off + lv.base, rec.key_len);
            const uint64_t row = d.query * F;
            bool inside = true;
            const Rank r = rank_of(d, start, lo, F, [&](uint32_t l2, uint64_t cnt, uint64_t *lb, bool *found) {
                if ((uint64_t)lo[row + l2] + cnt > levels[l2].n)
                    inside = false;
                bound_in_range(src, key, levels[l2], lo[row + l2], cnt, lb, found);
                if (*lb > cnt)
                    inside = false;
            });
            if (!inside)
                return fail("a bisection left its range: candidate", c, d.query, d.level);
            const uint64_t first = start[row];
            uint64_t slot;
            if (!slot_of(r, first, start[row + F] - first, &slot)) {
                if (compare)
                    return fail("the guard dropped a candidate of ascending levels", c, r.slot, first);
                continue;
            }
            if (slot >= C || slot < first || slot >= start[row + F])
                return fail("slot outside its query: candidate, slot, C", c, slot, C);
            if (compare && written[slot])
                return fail("two candidates in one slot", c, slot, 0);
            written[slot] = 1;
            slots[slot] = slot_value((uint32_t)c, r.superseded, zspack::is_delete(rec), keep);
        }
        /* the compaction, in slot order */
        std::vector<zscrc_zs_record> rows;
        std::vector<uint64_t> seqs, offs(nq + 1);
        uint64_t q = 0;
        for (uint64_t s = 0; s <= C; ++s) {
            while (q <= nq && start[q * F] == s)
                offs[q++] = rows.size();
            if (s == C)
                break;
            const uint32_t c = slots[s];
            if (c >= SLOT_DROPPED)
                continue;
            if (c >= C)
                return fail("a slot holds no candidate", s, c, C);
            const Cand d = decompose(start, lo, pairs, F, c);
            rows.push_back(row_of(levels[d.level], d.rec));
            seqs.push_back(firsts[d.level] + d.rec);
        }
        if (q != nq + 1)
            return fail("queries without an offset", q, nq, C);
        free(lo);
        free(start);
        free(slots);
        if (!compare)
            continue;
        if (rows.size() != m)
            return fail("row count differs: got, want, S", rows.size(), m, S);
        for (uint64_t i = 0; i <= nq; ++i)
            if (offs[i] != want_offs[i])
                return fail("offset differs at query, got, want", i, offs[i], want_offs[i]);
        for (uint64_t i = 0; i < m; ++i)
            if (memcmp(&rows[i], &want[i], 32) != 0 || seqs[i] != want_seq[i])
                return fail("row differs at row, S, seq", i, S, seqs[i]);
    }
    free(buf);
    free(qbuf);
    printf("ok %llu records %llu queries\n", (unsigned long long)n, (unsigned long long)nq);
    return 0;
}
