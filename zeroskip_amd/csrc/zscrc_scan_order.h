/*
 * zscrc_scan_order.h -- the arithmetic of the device prefix scan
 * (zscrc_device_scan, zscrc_scan.hip) and of its host form (zscrc_zs_scan):
 * the comparison of a prefix with a key cut to the prefix's length, the same
 * against a splitter table's two words, the end of a prefix's range in a level,
 * the decomposition of a candidate index into query, level and record, and the
 * rank of a candidate among its query's candidates with its guard.  Plain
 * inline functions, so the same definitions run in the kernels and in a CPU
 * program (tests/c/scan_order.cpp).
 *
 * The order is zscrc_merge_order.h's and the search zscrc_find_order.h's;
 * neither is restated here.  A prefix is a zsfind::Query; it is compared with
 * a key by handing the key over with its length cut to the prefix's, which
 * zsmerge::key_word pads with zeros from there on.  Under that comparison the
 * cut keys of an ascending level are smaller than the prefix (result 1 below:
 * the prefix is the greater), then equal to it -- the matches -- then greater
 * (result -1): the matches are the range from the prefix's lower bound to the
 * first key whose cut is greater.
 */
#ifndef ZSCRC_SCAN_ORDER_H
#define ZSCRC_SCAN_ORDER_H

#include <stdint.h>

#include "zscrc_find_order.h"

namespace zsscan {

using zsfind::Level;
using zsfind::Query;
using zsmerge::UNDECIDED;

/* what a slot holds instead of a candidate index */
constexpr uint32_t SLOT_SUPERSEDED = 0xFFFFFFFFu, SLOT_DROPPED = 0xFFFFFFFEu;

ZSREC_HD inline uint64_t cut(uint64_t klen, const Query &p) { return klen < p.len ? klen : p.len; }

/* The prefix against the key src[koff, +klen) cut to the prefix's length: 0 =
 * the key begins with the prefix; 1 = the cut key is smaller than the prefix
 * (a key shorter than the prefix that is a prefix of it among them); -1 = it
 * is greater. */
ZSREC_HD inline int cmp_prefix(const uint8_t *qsrc, const Query &p, const uint8_t *src, uint64_t koff, uint64_t klen)
{
    return zsfind::cmp_key(qsrc, p, src, koff, cut(klen, p));
}

/* A table entry's word at `at` (0 or 8) of a key of klen bytes, as the word of
 * the key cut to `len` bytes: zeros from byte len on. */
ZSREC_HD inline uint64_t cut_word(uint64_t w, uint64_t len, uint64_t at)
{
    if (len <= at)
        return 0;
    return len - at >= 8 ? w : w & ~(~0ull >> (8 * (len - at)));
}

/* cmp_prefix from a table entry: the key's words at 0 and 8, its length and
 * its rebased offset; the source is read only when 16 bytes leave it open. */
ZSREC_HD inline int cmp_prefix_words(const uint8_t *qsrc, const Query &p, const uint8_t *src, uint64_t w0, uint64_t w8,
                                     uint64_t klen, uint64_t koff)
{
    const uint64_t len = cut(klen, p);
    const int c = zsfind::cmp_words(p, cut_word(w0, len, 0), cut_word(w8, len, 8), len);
    return c != UNDECIDED ? c : zsfind::cmp_tail(qsrc, p, src, koff, len, 16);
}

/* The end of the prefix's range in a level: the first record at or after `lo`
 * (the prefix's lower bound, zsfind::find_in_level) with cmp_prefix -1, n if
 * there is none.  Through the table first (tab, S as in
 * find_in_level), then the records of the bucket.  The result lies in [lo, n]
 * whatever the level holds. */
ZSREC_HD inline uint64_t prefix_end(const uint8_t *qsrc, const Query &p, const uint8_t *src, const Level &lv,
                                    const uint64_t *tab, uint32_t S, uint64_t lo)
{
    uint64_t blo = 0, bhi = lv.n;
    bool unused = false;
    if (lo > lv.n)
        lo = lv.n;
    if (S > 1 && lv.n) {
        /* the splitters before the end compare 1 or 0: -1 is lower_bound's "not smaller" */
        const uint64_t t = zsfind::lower_bound(
            0, S,
            [&](uint64_t j) {
                return cmp_prefix_words(qsrc, p, src, tab[j], tab[2 * S + j], tab[S + j], tab[3 * S + j]) < 0 ? -1 : 1;
            },
            &unused);
        zsfind::bucket_bounds(t, lv.n, S, &blo, &bhi);
    }
    if (bhi < lo) /* only where the level does not ascend */
        bhi = lo;
    if (blo < lo)
        blo = lo;
    return zsfind::lower_bound(
        blo, bhi,
        [&](uint64_t i) {
            return cmp_prefix(qsrc, p, src, lv.recs[i].key_off + lv.base, lv.recs[i].key_len) < 0 ? -1 : 1;
        },
        &unused);
}

/* The candidates of a call are numbered query by query, inside a query level by
 * level (only levels that are not empty: F of them), inside a level by record:
 * pair e = query * F + level has the records [lo[e], lo[e] + start[e + 1] -
 * start[e]) and the candidates [start[e], start[e + 1]); start has pairs + 1
 * entries and ascends from 0. */
struct Cand {
    uint64_t pair;  /* query * F + level */
    uint64_t query;
    uint32_t level; /* among the levels that are not empty */
    uint64_t rec;   /* the record's index in its level */
};
struct Starts {
    const uint64_t *s;
    ZSREC_HD uint64_t operator[](uint64_t i) const { return s[i]; }
};
/* Candidate c < start[pairs], pairs = nq * F > 0. */
ZSREC_HD inline Cand decompose(const uint64_t *start, const uint32_t *lo, uint64_t pairs, uint32_t F, uint64_t c)
{
    Cand d;
    d.pair = zspack::find_rec(Starts{start}, pairs, c);
    d.query = d.pair / F;
    d.level = (uint32_t)(d.pair % F);
    d.rec = lo[d.pair] + (c - start[d.pair]);
    return d;
}

/* The rank of a candidate: its slot among its query's candidates sorted by
 * (key, level) and whether a newer level holds its key.  other(m, &lb, &found)
 * for every other level m of the query that has candidates: the lower bound of
 * the candidate's key among that level's candidates (0 .. their number) and
 * whether the key is there.  For ascending levels the slots of a query's
 * candidates are a permutation of [0, their number). */
struct Rank {
    uint64_t slot;
    bool superseded;
};
template <class Other>
ZSREC_HD inline Rank rank_of(const Cand &d, const uint64_t *start, const uint32_t *lo, uint32_t F, const Other &other)
{
    const uint64_t row = d.query * F;
    Rank r{d.rec - lo[d.pair], false};
    for (uint32_t m = 0; m < F; ++m) {
        const uint64_t cnt = start[row + m + 1] - start[row + m];
        if (m == d.level || !cnt)
            continue;
        uint64_t lb = 0;
        bool found = false;
        other(m, cnt, &lb, &found);
        r.slot += lb;
        if (found && m < d.level) {
            ++r.slot;
            r.superseded = true;
        }
    }
    return r;
}

/* The guard: the slot of the query's candidates [first, first + count) that a
 * rank names, false if it names none (only where a level does not ascend). */
ZSREC_HD inline bool slot_of(const Rank &r, uint64_t first, uint64_t count, uint64_t *slot)
{
    if (r.slot >= count)
        return false;
    *slot = first + r.slot;
    return true;
}

/* The lower bound of the key `key` (a Query over src) among the records [lo, lo
 * + cnt) of a level, relative to lo, and whether the key is there. */
ZSREC_HD inline void bound_in_range(const uint8_t *src, const Query &key, const Level &lv, uint64_t lo, uint64_t cnt,
                                    uint64_t *lb, bool *found)
{
    *found = false;
    *lb = zsfind::lower_bound(
              lo, lo + cnt,
              [&](uint64_t i) { return zsfind::cmp_key(src, key, src, lv.recs[i].key_off + lv.base, lv.recs[i].key_len); },
              found) -
          lo;
}

/* What a slot's candidate becomes. */
ZSREC_HD inline uint32_t slot_value(uint32_t c, bool superseded, bool is_delete, bool keep_deletes)
{
    return superseded ? SLOT_SUPERSEDED : is_delete && !keep_deletes ? SLOT_DROPPED : c;
}

/* A row: record `rec` of the level, rebased (checked before any scan). */
ZSREC_HD inline zscrc_zs_record row_of(const Level &lv, uint64_t rec)
{
    zscrc_zs_record r = lv.recs[rec];
    r.key_off += lv.base;
    if (!zspack::is_delete(r))
        r.val_off += lv.base;
    return r;
}

} /* namespace zsscan */

#endif
