/*
 * zscrc_records.h -- the record parsers that host and device share: the key /
 * delete record parser and the per-offset decision of zscrc_zs_records' loop
 * (zscrc_repack.cpp, built with the plain C++ compiler), the pointer section's
 * count and the packed file's two spans (zscrc_zs.cpp).  The kernels of
 * zscrc_device_records (zscrc_walk.hip) call the same definitions: every room
 * check is written once.
 *
 * Every length word comes from the file, which may be corrupt: each check is
 * against the bytes left (`room`), never an add that can wrap, and nothing
 * outside [img, img + size) is read.
 */
#ifndef ZSCRC_RECORDS_H
#define ZSCRC_RECORDS_H

#include <stdint.h>
#include <string.h>

#include "../../include/zscrc.h"

#ifdef __HIPCC__
#define ZSREC_HD __host__ __device__
#else
#define ZSREC_HD
#endif

namespace zsrec {

enum {
    T_KEY = 1, T_VALUE = 2, T_COMMIT = 4, T_2ND = 8, T_FINAL = 16, T_LONG = 32, T_DELETED = 64,
    T_LONG_KEY = T_KEY | T_LONG, T_LONG_COMMIT = T_COMMIT | T_LONG, T_LONG_FINAL = T_FINAL | T_LONG,
    T_LONG_DELETED = T_LONG, /* REC_TYPE_LONG_DELETED = LONG | LONG (zeroskip-priv.h:119) */
};

constexpr uint64_t HDR = 40;
constexpr uint64_t U64_MAX = ~0ull;

/* Big-endian 64-bit word at any byte address. */
ZSREC_HD inline uint64_t be64(const uint8_t *p)
{
#ifdef __HIP_DEVICE_COMPILE__
    if ((reinterpret_cast<uintptr_t>(p) & 7) == 0)
        return __builtin_bswap64(*reinterpret_cast<const uint64_t *>(p));
    uint64_t v = 0;
    for (int i = 0; i < 8; ++i)
        v = (v << 8) | p[i];
    return v;
#else
    uint64_t v;
    memcpy(&v, p, 8);
    return __builtin_bswap64(v);
#endif
}

ZSREC_HD inline uint64_t rup8(uint64_t n) { return (n + 7) & ~7ull; }

/* The key (and value) record at off, whose first word is w; size - off >= 8.
 * false if it is not one or does not fit the image.  r.val_off =
 * ZSCRC_ZS_DELETED for a delete record.  *next > off and *next <= size. */
ZSREC_HD inline bool record_at_w(const uint8_t *img, uint64_t size, uint64_t off, uint64_t w, zscrc_zs_record &r,
                                 uint64_t *next)
{
    const uint64_t room = size - off;
    const unsigned t = (unsigned)(w >> 56);
    if (t == T_KEY || t == T_LONG_KEY) {
        uint64_t klen, voff;
        if (t == T_KEY) {
            klen = (w >> 40) & 0xFFFF;
            voff = w & 0xFFFFFFFFull;
        } else {
            if (room < 24)
                return false;
            klen = be64(img + off + 8);
            voff = be64(img + off + 16);
        }
        if (klen > room - 24 || voff > room || room - voff < 16 || voff < 24 + klen)
            return false;
        const uint64_t v = off + voff;
        const uint64_t vw = be64(img + v);
        const uint64_t vlen = (vw >> 56) == T_VALUE ? ((vw >> 32) & 0xFFFFFF) : be64(img + v + 8);
        const uint64_t vroom = size - v - 16;
        if (vlen > vroom || rup8(vlen) > vroom)
            return false;
        r.key_off = off + 24;
        r.key_len = klen;
        r.val_off = v + 16;
        r.val_len = vlen;
        *next = v + 16 + rup8(vlen);
        return true;
    }
    if (t == T_DELETED || t == T_LONG_DELETED) {
        if (room < 24)
            return false;
        const uint64_t klen = t == T_DELETED ? ((w >> 40) & 0xFFFF) : be64(img + off + 8);
        if (klen > room - 24 || rup8(klen) > room - 24)
            return false;
        r.key_off = off + 24;
        r.key_len = klen;
        r.val_off = ZSCRC_ZS_DELETED;
        r.val_len = 0;
        *next = off + 24 + rup8(klen);
        return true;
    }
    return false;
}

/* The same at any off (a packed file's pointers are arbitrary bytes). */
ZSREC_HD inline bool record_at(const uint8_t *img, uint64_t size, uint64_t off, zscrc_zs_record &r, uint64_t *next)
{
    if (off > size || size - off < 8)
        return false;
    return record_at_w(img, size, off, be64(img + off), r, next);
}

/* What the record lister does at one offset of an active or finalised image. */
enum {
    L_SKIP = 0,   /* a commit record: go on at *next                         */
    L_RECORD = 1, /* a key or delete record in r: go on at *next             */
    L_TRUNC = 2,  /* a record runs past the end of the image                 */
    L_STOP = 3,   /* a record type the lister does not advance over          */
};

/* One iteration of the lister's loop at off < size; w = the word at off where
 * size - off >= 8 (not looked at otherwise).  L_SKIP / L_RECORD: *next > off
 * and *next <= size. */
ZSREC_HD inline int lister_step_w(const uint8_t *img, uint64_t size, uint64_t off, uint64_t w, zscrc_zs_record &r,
                                  uint64_t *next)
{
    if (size - off < 8)
        return L_TRUNC;
    const unsigned t = (unsigned)(w >> 56);
    if (t == T_COMMIT || t == T_LONG_COMMIT) {
        const uint64_t rl = t == T_COMMIT ? 8 : 24;
        if (size - off < rl)
            return L_TRUNC;
        *next = off + rl;
        return L_SKIP;
    }
    if (t != T_KEY && t != T_LONG_KEY && t != T_DELETED && t != T_LONG_DELETED)
        return L_STOP;
    return record_at_w(img, size, off, w, r, next) ? L_RECORD : L_TRUNC;
}

ZSREC_HD inline int lister_step(const uint8_t *img, uint64_t size, uint64_t off, zscrc_zs_record &r, uint64_t *next)
{
    return lister_step_w(img, size, off, size - off >= 8 ? be64(img + off) : 0, r, next);
}

/* An image in memory the caller can read directly: host memory on the host,
 * device memory in a kernel. */
struct Direct {
    const uint8_t *img;
    ZSREC_HD uint64_t word(uint64_t off) const { return be64(img + off); }
};

/* Length of the commit record at off and its span; false if not a commit.
 * Image: word(off) = the big-endian word at off. */
template <class Image>
ZSREC_HD inline bool commit_at(const Image &im, uint64_t size, uint64_t off, uint64_t *span_len, uint64_t *rec_len)
{
    if (off + 8 > size)
        return false;
    const uint64_t w = im.word(off);
    const unsigned t = (unsigned)(w >> 56);
    if (t == T_COMMIT || t == T_FINAL) {
        *span_len = (w >> 32) & 0xFFFFFF;
        *rec_len = 8;
    } else if (t == T_LONG_COMMIT || t == T_LONG_FINAL) {
        if (off + 24 > size)
            return false;
        *span_len = im.word(off + 8);
        *rec_len = 24;
    } else {
        return false;
    }
    return *span_len <= off;
}

/* zscrc_zs_packed_spans for an image behind any reader. */
template <class Image>
ZSREC_HD inline int packed_spans(const Image &im, uint64_t size, uint64_t span_off[2], uint64_t span_len[2])
{
    if (size < HDR + 16)
        return ZSCRC_EINVAL;
    /* final commit at the end: short FINAL, or LONG_FINAL whose 2ND_HALF word
     * ends the file (get_offset_to_pointers, zeroskip-packed.c:70-131) */
    uint64_t foff = size - 8;
    if ((im.word(foff) >> 56) == T_2ND)
        foff = size - 24;
    uint64_t sl, rl;
    if (!commit_at(im, size, foff, &sl, &rl) || rl != size - foff)
        return ZSCRC_ZS_TRUNCATED;
    const unsigned ft = (unsigned)(im.word(foff) >> 56);
    if (ft != T_FINAL && ft != T_LONG_FINAL)
        return ZSCRC_ZS_TRUNCATED;
    span_off[1] = foff - sl;
    span_len[1] = sl;
    /* the records-region commit ends where the pointer section starts */
    const uint64_t pstart = foff - sl;
    if (pstart < HDR + 8)
        return ZSCRC_ZS_TRUNCATED;
    uint64_t roff = pstart - 8;
    if ((im.word(roff) >> 56) == T_2ND && pstart >= HDR + 24)
        roff = pstart - 24;
    if (!commit_at(im, size, roff, &sl, &rl) || roff + rl != pstart)
        return ZSCRC_ZS_TRUNCATED;
    span_off[0] = roff - sl;
    span_len[0] = sl;
    return ZSCRC_OK;
}

/* The pointer section [poff, poff + plen) of a packed file: a BE64 count, then
 * that many BE64 record offsets.  false = the count does not fit the section. */
ZSREC_HD inline bool pointer_count(const uint8_t *img, uint64_t poff, uint64_t plen, uint64_t *count)
{
    *count = plen >= 8 ? be64(img + poff) : 0;
    return plen >= 8 && *count <= (plen - 8) / 8;
}

/* Pointer i (< the count) of the section at poff. */
ZSREC_HD inline uint64_t pointer_at(const uint8_t *img, uint64_t poff, uint64_t i)
{
    return be64(img + poff + 8 + 8 * i);
}

} /* namespace zsrec */

#endif
