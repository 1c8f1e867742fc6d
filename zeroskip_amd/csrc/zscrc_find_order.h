/*
 * zscrc_find_order.h -- the search arithmetic of the device lookup
 * (zscrc_device_find, zscrc_find.hip) and of its host form (zscrc_zs_find):
 * the query with its first two key words at hand, its comparison with a
 * record's key, the lower-bound bisection over an accessor, the positions of a
 * level's splitters, the bounds of the bucket a splitter search leaves, and
 * the whole search of one level.  Plain inline functions, so the same
 * definitions run in the kernels and in a CPU program (tests/c/find_order.cpp).
 *
 * The order is zscrc_merge_order.h's and is not restated here: a key is looked
 * at eight bytes at a time through zsmerge::key_word, and zsmerge::cmp_word
 * decides from two such words and the two lengths or asks for the next ones.
 */
#ifndef ZSCRC_FIND_ORDER_H
#define ZSCRC_FIND_ORDER_H

#include <stdint.h>

#include "zscrc_merge_order.h"

namespace zsfind {

using zsmerge::cmp_word;
using zsmerge::key_word;
using zsmerge::UNDECIDED;

constexpr uint32_t S_MAX = 2048; /* splitters of a level: a power of two, or 1 for none */

/* A key and its words at 0 and at 8: a query, or a record's key that is
 * compared with its neighbour. */
struct Query {
    uint64_t off, len, w0, w8;
};

/* The key [off, off + len) lies inside [0, size): against the bytes left. */
ZSREC_HD inline bool key_ok(uint64_t off, uint64_t len, uint64_t size) { return off <= size && len <= size - off; }

ZSREC_HD inline Query make_query(const uint8_t *qsrc, uint64_t off, uint64_t len)
{
    Query q;
    q.off = off;
    q.len = len;
    q.w0 = key_word(qsrc, off, len, 0);
    q.w8 = len > 8 ? key_word(qsrc, off, len, 8) : 0;
    return q;
}

/* The query against a key of klen bytes whose words at 0 and at 8 are w0 and
 * w8: -1, 0, 1, or UNDECIDED when both go on past byte 16 and are equal up to
 * there. */
ZSREC_HD inline int cmp_words(const Query &q, uint64_t w0, uint64_t w8, uint64_t klen)
{
    const int c = cmp_word(q.w0, q.len, w0, klen, 0);
    return c != UNDECIDED ? c : cmp_word(q.w8, q.len, w8, klen, 8);
}

/* The query against the key src[koff, +klen), both equal on their first `at`
 * bytes and longer than that. */
ZSREC_HD inline int cmp_tail(const uint8_t *qsrc, const Query &q, const uint8_t *src, uint64_t koff, uint64_t klen,
                             uint64_t at)
{
    for (;; at += 8) {
        const int c = cmp_word(key_word(qsrc, q.off, q.len, at), q.len, key_word(src, koff, klen, at), klen, at);
        if (c != UNDECIDED)
            return c;
    }
}

/* memcmp_raw of the query and the key src[koff, +klen). */
ZSREC_HD inline int cmp_key(const uint8_t *qsrc, const Query &q, const uint8_t *src, uint64_t koff, uint64_t klen)
{
    int c = cmp_word(q.w0, q.len, key_word(src, koff, klen, 0), klen, 0);
    if (c == UNDECIDED)
        c = cmp_word(q.w8, q.len, key_word(src, koff, klen, 8), klen, 8);
    return c != UNDECIDED ? c : cmp_tail(qsrc, q, src, koff, klen, 16);
}

/* Lower bound: the first i of [lo, hi) with cmp(i) <= 0, hi if there is none;
 * cmp(i) is the query against element i, and the elements ascend.  *equal:
 * cmp of the element returned is 0 (on entry: whether that holds for hi).
 * Where the elements do not ascend the result still lies in [lo, hi]. */
template <class Cmp>
ZSREC_HD inline uint64_t lower_bound(uint64_t lo, uint64_t hi, const Cmp &cmp, bool *equal)
{
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        const int c = cmp(mid);
        if (c > 0) {
            lo = mid + 1;
        } else {
            hi = mid;
            *equal = c == 0;
        }
    }
    return lo;
}

/* Splitter j (< S) of a level of n records (n > 0) is its record pos(j):
 * evenly spaced, ascending, pos(0) = 0; positions repeat where n < S. */
ZSREC_HD inline uint64_t splitter_pos(uint64_t j, uint64_t n, uint32_t S) { return j * n / S; }

/* t of the S splitters are smaller than the query (the lower bound among
 * them): the level's lower bound lies in [*lo, *hi] -- after the last smaller
 * splitter, at or before the first one that is not. */
ZSREC_HD inline void bucket_bounds(uint64_t t, uint64_t n, uint32_t S, uint64_t *lo, uint64_t *hi)
{
    *hi = t < S ? splitter_pos(t, n, S) : n;
    *lo = t ? splitter_pos(t - 1, n, S) + 1 : 0;
    if (*lo > *hi) /* only where the level does not ascend */
        *lo = *hi;
}

/* A level: n records whose offsets have `base` added (every one checked with
 * zsmerge::rebase before any search), and its splitter table, four arrays of S
 * words one after another (the words at 0, the lengths, the words at 8, the
 * rebased offsets); S = 1: no table. */
struct Level {
    const zscrc_zs_record *recs;
    uint64_t n;
    uint64_t base;
};

ZSREC_HD inline void table_store(uint64_t *tab, uint32_t S, uint32_t j, const uint8_t *src, uint64_t koff,
                                 uint64_t klen)
{
    tab[j] = key_word(src, koff, klen, 0);
    tab[S + j] = klen;
    tab[2 * S + j] = klen > 8 ? key_word(src, koff, klen, 8) : 0;
    tab[3 * S + j] = koff;
}

/* The number of the level's keys that are smaller than the query; *found: the
 * key at that index is the query.  tab: the level's table (the kernels: a copy
 * in LDS), read first; the source behind a splitter only when its two words
 * and the lengths leave the order undecided. */
ZSREC_HD inline uint64_t find_in_level(const uint8_t *qsrc, const Query &q, const uint8_t *src, const Level &lv,
                                       const uint64_t *tab, uint32_t S, bool *found)
{
    uint64_t lo = 0, hi = lv.n;
    *found = false;
    if (S > 1 && lv.n) {
        const uint64_t t = lower_bound(
            0, S,
            [&](uint64_t j) {
                const int c = cmp_words(q, tab[j], tab[2 * S + j], tab[S + j]);
                return c != UNDECIDED ? c : cmp_tail(qsrc, q, src, tab[3 * S + j], tab[S + j], 16);
            },
            found);
        bucket_bounds(t, lv.n, S, &lo, &hi);
    }
    return lower_bound(
        lo, hi,
        [&](uint64_t i) { return cmp_key(qsrc, q, src, lv.recs[i].key_off + lv.base, lv.recs[i].key_len); }, found);
}

/* What a search leaves of a query: the four words of zscrc_find_hit. */
struct Hit {
    uint64_t level, location, val_off, val_len;
};
constexpr uint64_t NONE = ~0ull, BAD_QUERY = ~0ull - 1;

/* Record `at` of level l holds the query. */
ZSREC_HD inline Hit hit_of(const Level &lv, uint64_t l, uint64_t at)
{
    const zscrc_zs_record r = lv.recs[at];
    return Hit{l, at, zspack::is_delete(r) ? r.val_off : r.val_off + lv.base, r.val_len};
}

/* Record j (> 0) of a level does not ascend from its predecessor, both inside
 * the source. */
ZSREC_HD inline bool order_offence(const uint8_t *src, const zscrc_zs_record &prev, const zscrc_zs_record &r)
{
    return cmp_key(src, make_query(src, prev.key_off, prev.key_len), src, r.key_off, r.key_len) >= 0;
}

/* The verdict of the check of the levels from its two minima, the smallest seq
 * of a record outside the source and the smallest one out of order (U64_MAX:
 * none): false = no offence, res untouched; else res[0] = ZSCRC_EINVAL, res[1]
 * the seq and res[7] which kind, a record outside the source first. */
ZSREC_HD inline bool check_verdict(uint64_t bad, uint64_t order, uint64_t *res)
{
    if (bad == zspack::U64_MAX && order == zspack::U64_MAX)
        return false;
    res[0] = (uint64_t)(int64_t)ZSCRC_EINVAL;
    res[1] = bad != zspack::U64_MAX ? bad : order;
    res[7] = bad == zspack::U64_MAX;
    return true;
}

} /* namespace zsfind */

#endif
