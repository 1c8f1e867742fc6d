/*
 * zscrc_next_order.h -- the arithmetic of the device successor stage
 * (zscrc_device_next, zscrc_next.hip) and of its host form (zscrc_zs_next): the
 * cursor a lower bound gives, the comparison of two levels' heads, one step of
 * the merge over an accessor for the cursors (the smallest key under them, the
 * 64-bit mask of the levels that hold it, the winner, the advance), the stop
 * rule, the filler, and the loop of one query built from them.  Plain inline
 * functions, so the same definitions run in the kernel and in a CPU program
 * (tests/c/next_order.cpp).
 *
 * The order is zscrc_merge_order.h's, the search zscrc_find_order.h's and the
 * row zscrc_scan_order.h's; none is restated here.  A level's head is the
 * record under its cursor; a cursor at or past the level's end has none.
 */
#ifndef ZSCRC_NEXT_ORDER_H
#define ZSCRC_NEXT_ORDER_H

#include <stdint.h>

#include "zscrc_scan_order.h"

namespace zsnext {

using zsfind::Level;
using zsfind::Query;

constexpr uint32_t PAGE_MAX = 65536;
/* the stop rule's "take another step": no state of a cursor */
constexpr uint64_t GO = ~0ull;

/* The cursor of a level from the query's lower bound there: the first key
 * greater than the query, with `inclusive` the first one not smaller. */
ZSREC_HD inline uint32_t cursor_of(uint64_t lb, bool found, bool inclusive)
{
    return (uint32_t)(lb + (found && !inclusive ? 1 : 0));
}

/* A level's head as a key with its first two words at hand. */
ZSREC_HD inline Query head_of(const uint8_t *src, const Level &lv, uint64_t at)
{
    return zsfind::make_query(src, lv.recs[at].key_off + lv.base, lv.recs[at].key_len);
}

/* memcmp_raw of the head `a` and record `at` of the level: both lie in src. */
ZSREC_HD inline int cmp_heads(const uint8_t *src, const Query &a, const Level &lv, uint64_t at)
{
    return zsfind::cmp_key(src, a, src, lv.recs[at].key_off + lv.base, lv.recs[at].key_len);
}

/* What a step takes: the key, the levels (bit l = level l of the F levels)
 * whose head is that key, the lowest of them and its record.  mask = 0: no
 * cursor has a record left. */
struct Step {
    Query key;
    uint64_t mask;
    uint32_t winner;
    uint32_t at;
};

/* The smallest key under the cursors: one pass over the levels that reads each
 * head.  level(l): level l as a Level; cur.get(l): its cursor.  Nothing moves. */
template <class Lv, class Cur>
ZSREC_HD inline Step pick(const uint8_t *src, uint32_t F, const Lv &level, const Cur &cur)
{
    Step st{Query{0, 0, 0, 0}, 0, F, 0};
    for (uint32_t l = 0; l < F; ++l) {
        const Level lv = level(l);
        const uint32_t c = cur.get(l);
        if (c >= lv.n)
            continue;
        /* > 0: the head so far is the greater one; the first level that holds the minimum stays the winner */
        const int cmp = st.mask ? cmp_heads(src, st.key, lv, c) : 1;
        if (cmp > 0) {
            st.key = head_of(src, lv, c);
            st.mask = 1ull << l;
            st.winner = l;
            st.at = c;
        } else if (cmp == 0) {
            st.mask |= 1ull << l;
        }
    }
    return st;
}

/* Every level that holds the step's key advances by one: at least the winner. */
template <class Cur>
ZSREC_HD inline void advance(uint32_t F, Cur &cur, const Step &st)
{
    for (uint32_t l = st.winner; l < F; ++l)
        if (st.mask >> l & 1)
            cur.set(l, cur.get(l) + 1);
}

/* The levels a step passed whose copy of the key lost. */
ZSREC_HD inline uint32_t superseded_of(const Step &st) { return (uint32_t)__builtin_popcountll(st.mask) - 1; }

/* The stop rule, before every step, in this order: the page is full; no cursor
 * has a record left; max_steps (0 = no limit) steps are taken.  GO = none. */
ZSREC_HD inline uint64_t stop_rule(uint64_t count, uint32_t page, bool left, uint64_t steps, uint32_t max_steps)
{
    if (count == page)
        return ZSCRC_NEXT_PAGE;
    if (!left)
        return ZSCRC_NEXT_END;
    if (max_steps && steps >= max_steps)
        return ZSCRC_NEXT_MORE;
    return GO;
}

/* What a slot past a query's rows holds, and its seq. */
ZSREC_HD inline zscrc_zs_record filler() { return zscrc_zs_record{ZSCRC_FIND_NONE, 0, 0, 0}; }
constexpr uint64_t FILLER_SEQ = ~0ull;

/* The cursor of a query whose key lies outside the query source. */
ZSREC_HD inline zscrc_next_cursor bad_cursor() { return zscrc_next_cursor{ZSCRC_FIND_NONE, 0, 0, ZSCRC_NEXT_BAD}; }

/* A query's share of the result words [2] .. [5], [8], [9]. */
struct Tally {
    uint64_t rows, steps, superseded, deletes, sumk, sumv;
};

/* One query from its cursors to its stop: emit(slot, row, level, record) for
 * every row in key order, slot = 0, 1, .. < page; the counts onto t; returns
 * what d_cur receives.  Every step advances a cursor that had a record left,
 * so the loop ends after at most n_total steps whatever the levels hold, and
 * no record outside [0, n) of its level is read. */
template <class Lv, class Cur, class Emit>
ZSREC_HD inline zscrc_next_cursor run_query(const uint8_t *src, uint32_t F, const Lv &level, Cur &cur, uint32_t page,
                                            uint32_t max_steps, bool keep_deletes, Tally &t, const Emit &emit)
{
    zscrc_next_cursor c{ZSCRC_FIND_NONE, 0, 0, 0};
    uint64_t steps = 0;
    for (;;) {
        Step st{Query{0, 0, 0, 0}, 0, F, 0};
        if (c.count < page)
            st = pick(src, F, level, cur);
        c.state = stop_rule(c.count, page, st.mask != 0, steps, max_steps);
        if (c.state != GO)
            break;
        advance(F, cur, st);
        ++steps;
        c.key_off = st.key.off;
        c.key_len = st.key.len;
        t.superseded += superseded_of(st);
        const zscrc_zs_record r = zsscan::row_of(level(st.winner), st.at);
        const bool del = zspack::is_delete(r);
        t.deletes += del;
        if (del && !keep_deletes)
            continue;
        emit((uint32_t)c.count, r, st.winner, st.at);
        ++c.count;
        t.sumk += r.key_len;
        if (!del)
            t.sumv += r.val_len;
    }
    if (c.state == ZSCRC_NEXT_END) {
        c.key_off = ZSCRC_FIND_NONE;
        c.key_len = 0;
    }
    t.steps += steps;
    t.rows += c.count;
    return c;
}

} /* namespace zsnext */

#endif
