/*
 * zscrc_merge_order.h -- the order arithmetic of the device merge
 * (zscrc_device_merge, zscrc_merge.hip): the rebase of a list's record into
 * the source with its bounds check, the 16-byte sort entry with its key
 * prefix, the comparator, the bitonic network's pairs, the merge-path diagonal
 * search and the winner rule.  Plain inline functions, so the same definitions
 * run in the kernels and in a CPU program (tests/c/merge_order.cpp).
 *
 * The order is the reference's memcmp_raw (zscrc_repack.cpp): unsigned bytes
 * over the shorter length, then the shorter key first; ties by the sequence
 * number, which is unique, so the order is total.
 *
 * A key is looked at eight bytes at a time, as the big-endian word of its
 * bytes [at, at + 8) with zeros past its end (key_word): one rule, cmp_word,
 * decides from two such words and the two lengths, or says that the next
 * words are needed.  The word at 0 lies in the sort entry, the tile sort keeps
 * the word at 8 beside it in LDS, every later one is read from the source with
 * the packer's gather (aligned 8-byte loads that hold at least one key byte).
 */
#ifndef ZSCRC_MERGE_ORDER_H
#define ZSCRC_MERGE_ORDER_H

#include <stdint.h>

#include "zscrc_pack_layout.h"

namespace zsmerge {

using zspack::is_delete;

/* A sort entry: the key's word at 0, the record's sequence number, its key
 * length cut to 32 bits (a longer key's length is read from its record). */
struct Entry {
    uint64_t prefix;
    uint32_t seq;
    uint32_t len;
};
constexpr uint32_t LEN_CAP = 0xFFFFFFFFu;
/* the entries that fill a tile past the input's end: after every record */
constexpr uint32_t SEQ_PAD = 0xFFFFFFFFu;
constexpr int UNDECIDED = 2;

/* The keys behind the entries: the source and the rebased records by seq. */
struct Keys {
    const uint8_t *src;
    const zscrc_zs_record *recs;
};

/* r of a list with `base`, moved into the source: false if its key or value
 * does not lie inside [0, src_size) then.  Every check is against the bytes
 * left. */
ZSREC_HD inline bool rebase(zscrc_zs_record &r, uint64_t base, uint64_t src_size)
{
    if (base > src_size || r.key_off > src_size - base)
        return false;
    r.key_off += base;
    if (r.key_len > src_size - r.key_off)
        return false;
    if (is_delete(r))
        return true;
    if (r.val_off > src_size - base)
        return false;
    r.val_off += base;
    return r.val_len <= src_size - r.val_off;
}

/* The big-endian word of the key's bytes [at, at + 8), zeros past its end. */
ZSREC_HD inline uint64_t key_word(const uint8_t *src, uint64_t off, uint64_t len, uint64_t at)
{
    if (at >= len)
        return 0;
    const uint64_t left = len - at;
    return __builtin_bswap64(zspack::gather8(src + off + at, left < 8 ? (uint32_t)left : 8));
}

ZSREC_HD inline Entry make_entry(const uint8_t *src, const zscrc_zs_record &r, uint32_t seq)
{
    Entry e;
    e.prefix = key_word(src, r.key_off, r.key_len, 0);
    e.seq = seq;
    e.len = r.key_len < LEN_CAP ? (uint32_t)r.key_len : LEN_CAP;
    return e;
}

/* Two keys that are equal on their first `at` bytes (both at least that
 * long), their words at `at` and their lengths (both cut at LEN_CAP or
 * neither): -1, 0, 1, or UNDECIDED when both go on past at + 8 with equal
 * words.  Equal words where the shorter key ends make it a prefix of the
 * other: its zero padding is the other's bytes. */
ZSREC_HD inline int cmp_word(uint64_t wa, uint64_t la, uint64_t wb, uint64_t lb, uint64_t at)
{
    if (wa != wb)
        return wa < wb ? -1 : 1;
    const uint64_t m = la < lb ? la : lb;
    if (m - at <= 8)
        return la < lb ? -1 : la > lb ? 1 : 0;
    return UNDECIDED;
}

/* The keys of records sa and sb, equal on their first `at` bytes and both
 * longer than that, compared from there on. */
ZSREC_HD inline int cmp_tail(const Keys &K, uint32_t sa, uint32_t sb, uint64_t at)
{
    const uint64_t oa = K.recs[sa].key_off, la = K.recs[sa].key_len;
    const uint64_t ob = K.recs[sb].key_off, lb = K.recs[sb].key_len;
    for (;; at += 8) {
        const int c = cmp_word(key_word(K.src, oa, la, at), la, key_word(K.src, ob, lb, at), lb, at);
        if (c != UNDECIDED)
            return c;
    }
}

/* memcmp_raw of the two entries' keys. */
ZSREC_HD inline int cmp_key(const Keys &K, const Entry &a, const Entry &b)
{
    const int c = cmp_word(a.prefix, a.len, b.prefix, b.len, 0);
    return c != UNDECIDED ? c : cmp_tail(K, a.seq, b.seq, 8);
}

/* mrec_less: by key, then by seq. */
ZSREC_HD inline bool less(const Keys &K, const Entry &a, const Entry &b)
{
    const int c = cmp_key(K, a, b);
    return c ? c < 0 : a.seq < b.seq;
}

/* The same with each key's word at 8 at hand (wa, wb), and with the padding
 * entries after every record. */
ZSREC_HD inline bool less_tile(const Keys &K, const Entry &a, uint64_t wa, const Entry &b, uint64_t wb)
{
    if (a.seq == SEQ_PAD || b.seq == SEQ_PAD)
        return a.seq != SEQ_PAD;
    int c = cmp_word(a.prefix, a.len, b.prefix, b.len, 0);
    if (c == UNDECIDED)
        c = cmp_word(wa, a.len, wb, b.len, 8);
    if (c == UNDECIDED)
        c = cmp_tail(K, a.seq, b.seq, 16);
    return c ? c < 0 : a.seq < b.seq;
}

/* Comparator t (< T / 2) of the bitonic network's step (k, j), k the size of
 * the sequences being merged and j the distance: it orders positions lo and
 * lo + j, ascending where `up`. */
ZSREC_HD inline void bitonic_pair(uint32_t t, uint32_t k, uint32_t j, uint32_t *lo, bool *up)
{
    *lo = 2 * t - (t & (j - 1));
    *up = (*lo & k) == 0;
}

/* Merge path: of the first d entries of the merge of the sorted runs a[0, na)
 * and b[0, nb), how many come from a (d <= na + nb; the order is total). */
template <class Run, class Less>
ZSREC_HD inline uint32_t diag_search(const Run &a, uint32_t na, const Run &b, uint32_t nb, uint32_t d,
                                     const Less &lt)
{
    uint32_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (lt(b[d - 1 - mid], a[mid]))
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

/* What becomes of entry i of the n sorted ones. */
enum { F_SUPERSEDED = 0, F_WINNER = 1, F_DROPPED = 2 };
ZSREC_HD inline int winner_flag(const Keys &K, const Entry *e, uint64_t i, uint64_t n, bool drop_deletes)
{
    if (i + 1 < n && cmp_key(K, e[i], e[i + 1]) == 0)
        return F_SUPERSEDED; /* a later record of the key replaces it */
    return drop_deletes && is_delete(K.recs[e[i].seq]) ? F_DROPPED : F_WINNER;
}

} /* namespace zsmerge */

#endif
