/*
 * zscrc_log_layout.h -- the layout arithmetic of an active log image that the
 * device log writer (zscrc_device_log, zscrc_devlog.hip) and its host twin
 * (zscrc_zs_log, zscrc_log.cpp) share.  A log is what zsdb_add / zsdb_remove /
 * zsdb_commit append to the active file: the records of a transaction, then
 * its commit record, 8 or 24 bytes by the length of its own CRC span.  Records
 * serialise as in a packed file (zscrc_pack_layout.h: rec_ok, rec_len,
 * piece_at, gather8, commit_words, header_words are used from there, not
 * copied); new here are the span rule, the two prefix sums a record's and a
 * commit's offset come from, and which record an output word falls into.
 * Plain inline functions, so the same definitions run in the kernels and in a
 * CPU program (tests/c/log_layout.cpp).
 *
 * Span rule (the reference's crc32_begin, src/zeroskip.c:930-931 and :985;
 * oracle/zs_format.py FileWriter): zsdb_add begins the span only where none is
 * open, zsdb_remove begins it always.  So the span a commit closes starts at
 * the transaction's LAST delete record if it has one, else at its first
 * record, and ends at the commit record.  An empty transaction has a span of
 * no bytes whose CRC is 0.
 *
 * With P[i] the bytes of the records before record i and C[t] the bytes of the
 * commit records before transaction t, record i of transaction t starts at
 * base + P[i] + C[t] and the commit of transaction t = [b, e) at
 * base + P[e] + C[t]; base = 40 for an image written from its header, else the
 * offset the call appends at.
 */
#ifndef ZSCRC_LOG_LAYOUT_H
#define ZSCRC_LOG_LAYOUT_H

#include <stdint.h>

#include "zscrc_pack_layout.h"

namespace zslog {

using zspack::commit_len;
using zspack::is_delete;
using zspack::MAX_SHORT_KEY_LEN;
using zspack::rec_len;
using zspack::rec_ok;
using zspack::sat_add;
using zsrec::HDR;
using zsrec::rup8;
using zsrec::U64_MAX;

/* Where a call may write from: 0 = a new image, header first; else an append
 * at a multiple of 8 behind a header. */
ZSREC_HD inline bool at_ok(uint64_t at) { return at == 0 || (at >= HDR && (at & 7) == 0); }
/* The offset of the first record or commit the call writes. */
ZSREC_HD inline uint64_t base_of(uint64_t at) { return at ? at : HDR; }

/* A record the log cannot hold: one outside the source, or a delete of a key
 * above 65,535 bytes (such a log cannot be walked: the oracle's delete_record,
 * SURVEY App. A). */
ZSREC_HD inline bool rec_bad(const zscrc_zs_record &r, uint64_t src_size)
{
    return !rec_ok(r, src_size) || (is_delete(r) && r.key_len > MAX_SHORT_KEY_LEN);
}

/* The delete mark of record i: i + 1 for a delete, 0 for any other record.
 * D[i], the largest mark of records 0..i, is "the largest delete index <= i"
 * plus one, 0 where there is none; marks combine by max. */
ZSREC_HD inline uint64_t del_mark(const zscrc_zs_record &r, uint64_t i) { return is_delete(r) ? i + 1 : 0; }
ZSREC_HD inline uint64_t mark_max(uint64_t a, uint64_t b) { return a > b ? a : b; }

/* Transaction t of a table of exclusive ends (NULL: one transaction a record). */
ZSREC_HD inline uint64_t tx_begin(const uint64_t *tx_end, uint64_t t) { return tx_end ? (t ? tx_end[t - 1] : 0) : t; }
ZSREC_HD inline uint64_t tx_stop(const uint64_t *tx_end, uint64_t t) { return tx_end ? tx_end[t] : t + 1; }
/* Entry t of a table of ntx entries over n records is in order. */
ZSREC_HD inline bool tx_ok(uint64_t b, uint64_t e, uint64_t t, uint64_t ntx, uint64_t n)
{
    return e >= b && e <= n && (t + 1 != ntx || e == n);
}
/* The transaction of record i: the first one that ends behind it (a checked
 * table whose last entry is n > i). */
ZSREC_HD inline uint64_t tx_of(const uint64_t *tx_end, uint64_t ntx, uint64_t i)
{
    if (!tx_end)
        return i;
    uint64_t lo = 0, hi = ntx; /* end[lo - 1] <= i, end[hi] > i */
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (tx_end[mid] <= i)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

/* The first record of the span of transaction [b, e): d_last = D[e - 1] (not
 * looked at for an empty transaction). */
ZSREC_HD inline uint64_t span_first(uint64_t b, uint64_t e, uint64_t d_last)
{
    return e > b && d_last > b ? d_last - 1 : b;
}
/* Its length from the byte prefix P at its first record and at e. */
ZSREC_HD inline uint64_t span_bytes(uint64_t p_first, uint64_t p_e) { return p_e - p_first; }

/* File offsets from the two prefix sums; every term saturates. */
ZSREC_HD inline uint64_t placed(uint64_t base, uint64_t p, uint64_t c) { return sat_add(sat_add(base, p), c); }

/* The sizes of a call: R = the records' bytes, ctot = the commit bytes of its
 * ntx transactions, finalise: one more short commit. */
struct Totals {
    uint64_t body_end; /* behind the last transaction's commit */
    uint64_t end;      /* the new file size */
    uint64_t written;  /* bytes the call writes, the header included */
    uint64_t commits, long_commits;
};
ZSREC_HD inline Totals totals(uint64_t at, uint64_t R, uint64_t ctot, uint64_t ntx, bool finalise)
{
    Totals t;
    t.body_end = placed(base_of(at), R, ctot);
    t.end = sat_add(t.body_end, finalise ? 8 : 0);
    t.written = t.end == U64_MAX ? U64_MAX : t.end - at;
    t.commits = ntx + (finalise ? 1 : 0);
    t.long_commits = (ctot - 8 * ntx) / 16; /* 8 a short one, 24 a long one */
    return t;
}

/* Record i as the lister finds it in the written bytes, from its start. */
ZSREC_HD inline zscrc_zs_record listed(const zscrc_zs_record &r, uint64_t start)
{
    zscrc_zs_record o;
    o.key_off = start + 24;
    o.key_len = r.key_len;
    const bool del = is_delete(r);
    o.val_off = del ? ZSCRC_ZS_DELETED : start + 24 + rup8(r.key_len) + 16;
    o.val_len = del ? 0 : r.val_len;
    return o;
}

/* Whether the 8-byte word at file offset p belongs to the record r that starts
 * at `start` (the last start at or before p, if any): *rel = its offset in the
 * record.  false: p lies before the first record or in the commit record(s)
 * behind r, whose words come from the span CRCs. */
ZSREC_HD inline bool word_in_rec(const zscrc_zs_record &r, uint64_t start, uint64_t p, uint64_t *rel)
{
    if (p < start)
        return false;
    *rel = p - start;
    return *rel < rec_len(r);
}

/* 40 + 54 n + 24 n_commits + sum_key_len + sum_val_len, 0 if that wraps: a
 * record takes at most 24 + 7 + 16 + 7 bytes beside its key and value. */
inline uint64_t bound(uint64_t n, uint64_t n_commits, uint64_t sum_key_len, uint64_t sum_val_len)
{
    uint64_t b, c;
    if (__builtin_mul_overflow(n, (uint64_t)54, &b) || __builtin_mul_overflow(n_commits, (uint64_t)24, &c) ||
        __builtin_add_overflow(b, c, &b) || __builtin_add_overflow(b, HDR, &b) ||
        __builtin_add_overflow(b, sum_key_len, &b) || __builtin_add_overflow(b, sum_val_len, &b))
        return 0;
    return b;
}

/* What the entry points refuse before any work (zscrc_device_log's list, less
 * the pointers' alignment and overlap, which are the device's). */
constexpr uint64_t N_MAX = (1ull << 31) - 1;
inline bool counts_ok(uint64_t n, uint64_t n_tx, uint64_t src_size)
{
    return n <= N_MAX && n_tx <= N_MAX && src_size <= zspack::SRC_MAX;
}

} /* namespace zslog */

#endif
