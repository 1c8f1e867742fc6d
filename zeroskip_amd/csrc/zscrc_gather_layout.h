/*
 * zscrc_gather_layout.h -- the arithmetic of the value gather that the kernels
 * of zscrc_gather.hip and the host twin (zscrc_zs_gather) share: what an item
 * is (a value, a delete, a key that was not found, a bad query), whether its
 * value lies inside the source, the length it adds to the output, and the
 * builder of output words from source bytes at any alignment.  Plain inline
 * functions, so the same definitions run in the kernels and in a CPU program
 * (tests/c/gather_layout.cpp).
 *
 * An item is four 64-bit words, of which 0, 2 and 3 are read: a zscrc_find_hit
 * {level, location, val_off, val_len} or a zscrc_zs_record {key_off, key_len,
 * val_off, val_len}.  The output is the values back to back in item order;
 * offs[i] is the start of item i's value there and offs[n] the total, so an
 * item without a value, or with an empty one, has offs[i + 1] == offs[i].
 */
#ifndef ZSCRC_GATHER_LAYOUT_H
#define ZSCRC_GATHER_LAYOUT_H

#include <stdint.h>

#include "zscrc_pack_layout.h"

namespace zsgather {

using zspack::gather8;
using zspack::sat_add;
using zspack::U64_MAX;

enum Kind { VALUE = 0, DELETED = 1, NOT_FOUND = 2, BAD_QUERY = 3, KINDS = 4 };

/* What the item with these words 0 and 2 is.  A record's word 0 is a key
 * offset, below 2^62, so a record is a value or a delete. */
ZSREC_HD inline Kind kind_of(uint64_t w0, uint64_t val_off)
{
    if (w0 == ZSCRC_FIND_BAD_QUERY)
        return BAD_QUERY;
    if (w0 == ZSCRC_FIND_NONE)
        return NOT_FOUND;
    return val_off == ZSCRC_ZS_DELETED ? DELETED : VALUE;
}

/* The value [val_off, +val_len) lies inside [0, src_size): against the bytes
 * left, never with an add that can wrap. */
ZSREC_HD inline bool value_ok(uint64_t val_off, uint64_t val_len, uint64_t src_size)
{
    return val_off <= src_size && val_len <= src_size - val_off;
}

/* The bytes an item adds to the output. */
ZSREC_HD inline uint64_t len_of(Kind k, uint64_t val_len) { return k == VALUE ? val_len : 0; }

/* Sums of lengths saturate at UINT64_MAX instead of wrapping. */
ZSREC_HD inline uint64_t sum_len(uint64_t a, uint64_t b) { return sat_add(a, b); }

/* The n (1..8) output bytes at [p, p + n), p + n <= offs[count], as a word
 * (first byte = lowest 8 bits, the rest zero).  offs[i]: the start of item i
 * in the output; val_off(i): its value's offset in src.  j: on entry an item
 * with offs[j] <= p that is not past the item holding byte p, on return the
 * item that holds byte p + n - 1 -- what the word at p + n takes.  Items
 * without bytes in between are stepped over, however many there are; only
 * aligned 8-byte source words that hold a byte of a value are read. */
template <class Offs, class ValOff>
ZSREC_HD inline uint64_t build8(const uint8_t *src, const Offs &offs, const ValOff &val_off, uint64_t &j, uint64_t p,
                                uint32_t n)
{
    uint64_t v = 0;
    uint32_t got = 0;
    for (;;) {
        const uint64_t at = p + got, end = offs[j + 1], left = end > at ? end - at : 0;
        const uint32_t m = left < n - got ? (uint32_t)left : n - got;
        if (m)
            v |= gather8(src + val_off(j) + (at - offs[j]), m) << (8 * got);
        got += m;
        if (got == n)
            return v;
        ++j;
    }
}

} /* namespace zsgather */

#endif
