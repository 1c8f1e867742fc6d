/*
 * next_order.cpp -- the device successor stage's arithmetic on the CPU
 * (tests/test_next_order.py).  Includes only the header the kernels of
 * zscrc_next.hip share with the host, reads a case file
 *
 *   u64 src_len, k, n_total, qsrc_len, nq, shift, qshift, page, flags,
 *       max_steps, compare;
 *   k x (u64 n, base); src[src_len]; recs[n_total] (4 x u64, not rebased);
 *   qsrc[qsrc_len]; queries[nq] (4 x u64);
 *   compare != 0: rows[nq * page] (4 x u64); seqs[nq * page]; cur[nq] (4 x
 *   u64); res[12]          (compare = 0: nothing follows and the levels need
 *                           not ascend)
 *
 * and runs the stage the way the kernels do, at 1, 2, 64, 1,024 (the default)
 * and 2,048 splitters: every record rebased and checked, every level's table,
 * the cursor of every (level, query) pair through the table -- which must
 * equal the cursor without one -- into a level-major matrix, then every query
 * through zsnext::run_query, the filler and the sums.  Every position is
 * checked against its array before it is used, and the arrays are exact
 * allocations, so a sanitizer sees what the checks miss.  A query may take at
 * most n_total steps.  The source and the query bytes lie at addresses = shift
 * and qshift mod 8 in allocations that end with their last 8-byte granule.
 * Exit status 0 = rows, seqs, cursors and result words equal the expected
 * ones at every table size.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../zeroskip_amd/csrc/zscrc_next_order.h"

using namespace zsfind;
using namespace zsnext;

static int fail(const char *what, uint64_t a, uint64_t b, uint64_t c)
{
    fprintf(stderr, "next_order: %s (%llu, %llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b,
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

/* Query i's column of the level-major matrix, every access checked. */
struct Column {
    uint32_t *m;
    uint64_t nq, i, F;
    bool *outside;
    uint32_t get(uint32_t l) const
    {
        if (l >= F) {
            *outside = true;
            return ~0u;
        }
        return m[l * nq + i];
    }
    void set(uint32_t l, uint32_t v)
    {
        if (l >= F)
            *outside = true;
        else
            m[l * nq + i] = v;
    }
};

int main(int argc, char **argv)
{
    if (argc != 2)
        return fail("usage: next_order CASEFILE", 0, 0, 0);
    FILE *f = fopen(argv[1], "rb");
    uint64_t hd[11];
    if (!f || fread(hd, 8, 11, f) != 11)
        return fail("cannot read the case", 0, 0, 0);
    const uint64_t src_len = hd[0], k = hd[1], n = hd[2], qsrc_len = hd[3], nq = hd[4], shift = hd[5] & 7,
                   qshift = hd[6] & 7, page = hd[7], flags = hd[8];
    const uint32_t max_steps = (uint32_t)hd[9];
    const bool compare = hd[10] != 0, inclusive = flags & ZSCRC_NEXT_INCLUSIVE, keep = flags & ZSCRC_NEXT_KEEP_DELETES;
    if (!page || page > PAGE_MAX)
        return fail("bad page", page, 0, 0);
    const uint64_t slots = nq * page;
    std::vector<uint64_t> lists(2 * k);
    uint8_t *buf = granules(shift, src_len), *qbuf = granules(qshift, qsrc_len);
    uint8_t *src = buf + shift, *qsrc = qbuf + qshift;
    std::vector<zscrc_zs_record> recs(n), queries(nq), want(compare ? slots : 0);
    std::vector<uint64_t> want_seq(compare ? slots : 0), want_res(ZSCRC_NEXT_RES_WORDS);
    std::vector<zscrc_next_cursor> want_cur(compare ? nq : 0);
    if (k && fread(lists.data(), 16, k, f) != k)
        return fail("short case file: lists", k, 0, 0);
    if ((src_len && fread(src, 1, src_len, f) != src_len) || (n && fread(recs.data(), 32, n, f) != n))
        return fail("short case file: source and records", src_len, n, 0);
    if ((qsrc_len && fread(qsrc, 1, qsrc_len, f) != qsrc_len) || (nq && fread(queries.data(), 32, nq, f) != nq))
        return fail("short case file: queries", qsrc_len, nq, 0);
    if (compare && ((slots && fread(want.data(), 32, slots, f) != slots) ||
                    (slots && fread(want_seq.data(), 8, slots, f) != slots) ||
                    (nq && fread(want_cur.data(), 32, nq, f) != nq) ||
                    fread(want_res.data(), 8, ZSCRC_NEXT_RES_WORDS, f) != ZSCRC_NEXT_RES_WORDS))
        return fail("short case file: expected words", slots, nq, 0);
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
        /* the bounds launches: the cursors, level major */
        uint32_t *matrix = exact<uint32_t>((uint64_t)F * nq);
        for (uint32_t l = 0; l < F; ++l)
            for (uint64_t i = 0; i < nq; ++i) {
                if (!key_ok(queries[i].key_off, queries[i].key_len, qsrc_len)) {
                    matrix[l * nq + i] = 0xDEADBEEFu; /* never read */
                    continue;
                }
                const Query q = make_query(qsrc, queries[i].key_off, queries[i].key_len);
                bool found, plain_found;
                const uint64_t lb = find_in_level(qsrc, q, src, levels[l], tabs[l].data(), S, &found);
                const uint64_t pl = find_in_level(qsrc, q, src, levels[l], nullptr, 1, &plain_found);
                const uint32_t c = cursor_of(lb, found, inclusive);
                if (compare && c != cursor_of(pl, plain_found, inclusive))
                    return fail("the cursors through the table and without differ: query, level, S", i, l, S);
                if (c > levels[l].n)
                    return fail("cursor outside the level: query, level, cursor", i, l, c);
                matrix[l * nq + i] = c;
            }
        /* the step launch */
        zscrc_zs_record *rows = exact<zscrc_zs_record>(slots);
        uint64_t *seqs = exact<uint64_t>(slots);
        zscrc_next_cursor *cur = exact<zscrc_next_cursor>(nq);
        uint64_t res[ZSCRC_NEXT_RES_WORDS] = {0, nq};
        Tally t{0, 0, 0, 0, 0, 0};
        for (uint64_t i = 0; i < nq; ++i) {
            zscrc_next_cursor c = bad_cursor();
            bool outside = false;
            if (!key_ok(queries[i].key_off, queries[i].key_len, qsrc_len)) {
                ++res[6];
            } else {
                Column col{matrix, nq, i, F, &outside};
                const uint64_t steps_before = t.steps;
                c = run_query(
                    src, F,
                    [&](uint32_t l) {
                        if (l >= F) {
                            outside = true;
                            return Level{nullptr, 0, 0};
                        }
                        return levels[l];
                    },
                    col, (uint32_t)page, max_steps, keep, t,
                    [&](uint32_t slot, const zscrc_zs_record &r, uint32_t l, uint32_t at) {
                        if (slot >= page || l >= F || at >= levels[l].n) {
                            outside = true;
                            return;
                        }
                        rows[i * page + slot] = r;
                        seqs[i * page + slot] = firsts[l] + at;
                    });
                if (t.steps - steps_before > n)
                    return fail("more steps than records: query, steps, n", i, t.steps - steps_before, n);
                if (max_steps && t.steps - steps_before > max_steps)
                    return fail("more steps than max_steps: query, steps", i, t.steps - steps_before, max_steps);
                for (uint32_t l = 0; l < F; ++l)
                    if (matrix[l * nq + i] > levels[l].n)
                        return fail("a cursor left its level: query, level, cursor", i, l, matrix[l * nq + i]);
                res[10] += c.state == ZSCRC_NEXT_END;
                res[11] += c.state == ZSCRC_NEXT_MORE;
            }
            if (outside || c.count > page)
                return fail("a position outside its array: query, count", i, c.count, page);
            for (uint64_t slot = c.count; slot < page; ++slot) {
                rows[i * page + slot] = filler();
                seqs[i * page + slot] = FILLER_SEQ;
            }
            cur[i] = c;
        }
        res[2] = t.rows;
        res[3] = t.steps;
        res[4] = t.superseded;
        res[5] = t.deletes;
        res[8] = t.sumk;
        res[9] = t.sumv;
        int rc = 0;
        if (compare) {
            for (uint64_t i = 0; i < nq && !rc; ++i)
                if (memcmp(&cur[i], &want_cur[i], 32) != 0)
                    rc = fail("cursor differs at query, S, state", i, S, cur[i].state);
            for (uint64_t i = 0; i < slots && !rc; ++i)
                if (memcmp(&rows[i], &want[i], 32) != 0 || seqs[i] != want_seq[i])
                    rc = fail("row differs at slot, S, seq", i, S, seqs[i]);
            for (uint64_t i = 0; i < ZSCRC_NEXT_RES_WORDS && !rc; ++i)
                if (res[i] != want_res[i])
                    rc = fail("result word differs: word, got, want", i, res[i], want_res[i]);
        }
        free(matrix);
        free(rows);
        free(seqs);
        free(cur);
        if (rc)
            return rc;
    }
    free(buf);
    free(qbuf);
    printf("ok %llu records %llu queries\n", (unsigned long long)n, (unsigned long long)nq);
    return 0;
}
