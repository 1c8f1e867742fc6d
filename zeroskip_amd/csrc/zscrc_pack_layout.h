/*
 * zscrc_pack_layout.h -- the layout arithmetic of a packed file that the host
 * and the device packer (zscrc_device_pack, zscrc_devpack.hip) share: the
 * serialised length of a record, the sections of the file, the tiles the
 * records region is cut into, which piece of which record an output word falls
 * into and at what source offset, the gather of source bytes from any
 * alignment, and the commit records and header with their host-order CRCs.
 * Plain inline functions, so the same definitions run in the kernels and in a
 * CPU program (tests/c/pack_layout.cpp).
 *
 * Byte layout: zscrc_pack.cpp (the host writer; the reference's
 * zs_packed_file_new_from_memtree, src/zeroskip-packed.c:384-473).
 *
 * Record lengths come from the caller's list, which may be wrong: a record is
 * checked against the bytes left of the source (rec_ok), never with an add
 * that can wrap, and sums saturate (sat_add) instead of wrapping.
 */
#ifndef ZSCRC_PACK_LAYOUT_H
#define ZSCRC_PACK_LAYOUT_H

#include <stdint.h>

#include "zscrc_records.h"

namespace zspack {

using zsrec::HDR;
using zsrec::rup8;
using zsrec::U64_MAX;

constexpr uint64_t MAX_SHORT_KEY_LEN = 65535;    /* zeroskip-priv.h */
constexpr uint64_t MAX_SHORT_VAL_LEN = 16777215; /* zeroskip-priv.h:171 */
constexpr uint64_t SIGNATURE = 0x5a45524f534b4950ull;
constexpr uint32_t VERSION = 1;
/* A source of more bytes is refused by the entry point: below it the length
 * of one valid record cannot wrap. */
constexpr uint64_t SRC_MAX = 1ull << 62;

ZSREC_HD inline uint64_t sat_add(uint64_t a, uint64_t b) { return a + b < a ? U64_MAX : a + b; }

ZSREC_HD inline bool is_delete(const zscrc_zs_record &r) { return r.val_off == ZSCRC_ZS_DELETED; }

/* Key and value lie inside [0, src_size). */
ZSREC_HD inline bool rec_ok(const zscrc_zs_record &r, uint64_t src_size)
{
    if (r.key_off > src_size || r.key_len > src_size - r.key_off)
        return false;
    return is_delete(r) || (r.val_off <= src_size && r.val_len <= src_size - r.val_off);
}

/* Serialised length of a record that is rec_ok for a source of at most SRC_MAX bytes. */
ZSREC_HD inline uint64_t rec_len(const zscrc_zs_record &r)
{
    return 24 + rup8(r.key_len) + (is_delete(r) ? 0 : 16 + rup8(r.val_len));
}

/* Length of the commit record that closes a span. */
ZSREC_HD inline uint64_t commit_len(uint64_t span) { return span <= MAX_SHORT_VAL_LEN ? 8 : 24; }

/* The sections of the packed file of n records whose records region has
 * region bytes: header [0, 40), region [40, 40 + region), its commit, the
 * pointer section at ptr_off (count + n pointers), the final commit.  Every
 * field saturates at UINT64_MAX. */
struct Layout {
    uint64_t region, ptr_off, ptr_bytes, file_bytes;
};
ZSREC_HD inline Layout layout(uint64_t n, uint64_t region)
{
    Layout l;
    l.region = region;
    l.ptr_off = sat_add(sat_add(HDR, region), commit_len(region));
    l.ptr_bytes = n >= (U64_MAX >> 3) ? U64_MAX : 8 * (n + 1);
    l.file_bytes = sat_add(sat_add(l.ptr_off, l.ptr_bytes), commit_len(l.ptr_bytes));
    return l;
}

/* Output tiles: tile t is the file offsets [t * tile, (t + 1) * tile) cut to
 * the records region, so every 16-byte word of a tile is 16-byte aligned in a
 * 16-byte aligned output.  In region coordinates (file offset - 40); the copy
 * itself sweeps in file coordinates (zscrc_copy_tiles.h), and
 * tests/c/pack_layout.cpp holds the two against each other: */
ZSREC_HD inline uint64_t tile_count(uint64_t tile, uint64_t region) { return (HDR + region + tile - 1) / tile; }
ZSREC_HD inline void tile_range(uint64_t t, uint64_t tile, uint64_t region, uint64_t *lo, uint64_t *hi)
{
    const uint64_t a = t * tile, b = a + tile;
    *lo = a < HDR ? 0 : a - HDR;
    *hi = b - HDR < region ? b - HDR : region;
}

/* The largest j < m with start[j] <= p; start ascending, start[0] <= p. */
template <class Starts>
ZSREC_HD inline uint64_t find_rec(const Starts &start, uint64_t m, uint64_t p)
{
    uint64_t lo = 0, hi = m; /* start[lo] <= p, start[hi] > p (hi = m: none) */
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (start[mid] <= p)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

/* An 8-byte output word as it lies in memory (first byte = lowest 8 bits). */
ZSREC_HD inline uint64_t mem_be64(uint64_t v) { return __builtin_bswap64(v); }

/* The output word at rel (a multiple of 8, < rec_len(r)) of a record: n = 0:
 * the generated word `word`; else the n (1..8) source bytes at src_off
 * followed by 8 - n zero bytes. */
struct Piece {
    uint64_t word;
    uint64_t src_off;
    uint32_t n;
};
ZSREC_HD inline Piece piece_at(const zscrc_zs_record &r, uint64_t rel)
{
    using namespace zsrec;
    const uint64_t klen = r.key_len, kpad = rup8(klen), kbuflen = 24 + kpad;
    const bool del = is_delete(r);
    Piece p{0, 0, 0};
    if (rel < 24) {
        const bool lng = klen > MAX_SHORT_KEY_LEN;
        uint64_t w;
        if (rel == 0) {
            /* a long delete leaves its first word zero, as the reference does */
            w = del ? (lng ? 0 : ((uint64_t)T_DELETED << 56) | (klen << 40))
                    : (lng ? (uint64_t)T_LONG_KEY << 56 : ((uint64_t)T_KEY << 56) | (klen << 40) | kbuflen);
        } else if (rel == 8) {
            w = lng ? klen : 0;
        } else {
            w = lng && !del ? kbuflen : 0;
        }
        p.word = mem_be64(w);
        return p;
    }
    if (rel < kbuflen) {
        const uint64_t at = rel - 24, left = klen - at;
        p.src_off = r.key_off + at;
        p.n = left < 8 ? (uint32_t)left : 8;
        return p;
    }
    const uint64_t v = rel - kbuflen, vlen = r.val_len;
    if (v < 16) {
        const bool lng = vlen > MAX_SHORT_VAL_LEN;
        const uint64_t w = v == 0 ? (lng ? (uint64_t)(T_VALUE | T_LONG) << 56 : ((uint64_t)T_VALUE << 56) | (vlen << 32))
                                  : (lng ? vlen : 0);
        p.word = mem_be64(w);
        return p;
    }
    const uint64_t at = v - 16, left = vlen - at;
    p.src_off = r.val_off + at;
    p.n = left < 8 ? (uint32_t)left : 8;
    return p;
}

/* The n (1..8) bytes at p, any alignment, then zeros: two aligned 8-byte loads
 * and a byte shift.  Only aligned words that hold at least one of the n bytes
 * are read (the second one only when the bytes reach into it). */
ZSREC_HD inline uint64_t gather8(const uint8_t *p, uint32_t n)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const unsigned sh = (unsigned)(a & 7) * 8;
    const uint64_t *w = reinterpret_cast<const uint64_t *>(a & ~(uintptr_t)7);
    uint64_t v = w[0] >> sh;
    if (sh + 8 * n > 64)
        v |= w[1] << (64 - sh);
    return n >= 8 ? v : v & ((1ull << (8 * n)) - 1);
}

/* crc32c continued over the 8 bytes of a host-order word (the rule of
 * commit_record() in zscrc_pack.cpp: trailer words are hashed as they lie in
 * the host's memory, little-endian here and on the device). */
ZSREC_HD inline uint32_t crc_bytes(uint32_t crc, uint64_t w, int nbytes)
{
    crc = ~crc;
    for (int i = 0; i < nbytes; ++i) {
        crc ^= (uint32_t)(w >> (8 * i)) & 0xFF;
        for (int k = 0; k < 8; ++k)
            crc = (crc >> 1) ^ (0x82F63B78u & (0u - (crc & 1)));
    }
    return ~crc;
}

/* The commit record closing a span of span_len bytes whose crc32c(0, span) is
 * span_crc, as output words; returns their number (1 or 3), *stored = its CRC. */
ZSREC_HD inline int commit_words(uint32_t span_crc, uint64_t span_len, bool final, uint64_t out[3], uint32_t *stored)
{
    using namespace zsrec;
    if (span_len > MAX_SHORT_VAL_LEN) {
        const uint64_t t1 = (uint64_t)(final ? T_LONG_FINAL : T_LONG_COMMIT) << 56;
        const uint64_t t2 = (uint64_t)T_2ND << 56;
        uint32_t c = crc_bytes(span_crc, t1, 8);
        c = crc_bytes(c, span_len, 8);
        c = crc_bytes(c, t2, 8);
        out[0] = mem_be64(t1);
        out[1] = mem_be64(span_len);
        out[2] = mem_be64(t2 | c);
        *stored = c;
        return 3;
    }
    const uint64_t w = ((uint64_t)(final ? T_FINAL : T_COMMIT) << 56) | (span_len << 32);
    const uint32_t c = crc_bytes(span_crc, w, 8);
    out[0] = mem_be64(w | c);
    *stored = c;
    return 1;
}

/* The 40-byte header as five output words, its CRC over the host-order
 * fields (zeroskip-header.c:30-94; zscrc_pack_open). */
struct Header {
    uint64_t w[5];
};
ZSREC_HD inline Header header_words(const uint8_t uuid[16], uint32_t startidx, uint32_t endidx)
{
    uint64_t u0 = 0, u1 = 0;
    for (int i = 0; i < 8; ++i) {
        u0 |= (uint64_t)uuid[i] << (8 * i);
        u1 |= (uint64_t)uuid[8 + i] << (8 * i);
    }
    uint32_t c = crc_bytes(0, SIGNATURE, 8);
    c = crc_bytes(c, VERSION, 4);
    c = crc_bytes(c, u0, 8);
    c = crc_bytes(c, u1, 8);
    c = crc_bytes(c, startidx, 4);
    c = crc_bytes(c, endidx, 4);
    /* bytes: signature (native order), BE32 version, uuid, BE32 startidx, endidx, crc */
    const uint64_t ver = __builtin_bswap32(VERSION), st = __builtin_bswap32(startidx),
                   en = __builtin_bswap32(endidx), cc = __builtin_bswap32(c);
    Header h;
    h.w[0] = SIGNATURE;
    h.w[1] = ver | (u0 << 32);
    h.w[2] = (u0 >> 32) | (u1 << 32);
    h.w[3] = (u1 >> 32) | (st << 32);
    h.w[4] = en | (cc << 32);
    return h;
}

} /* namespace zspack */

#endif
