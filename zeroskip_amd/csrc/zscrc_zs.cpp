/*
 * zscrc_zs.cpp -- zeroskip file images -> commit span descriptors -> GPU
 * verification (the "next" row of SURVEY.md sec 8f: verify-on-open,
 * `consistent`, repack re-checksum).
 *
 * The record walk is the reference's, restated for the checksum parts only:
 *   walk            src/zeroskip-record.c:283-331 (stops, like the reference,
 *                   at record types it does not advance over)
 *   key + value     src/zeroskip-record.c:75-106,156-181 (value offset from
 *                   the key word, value length from the value word)
 *   delete          src/zeroskip-record.c:183-199 (uint16 key length)
 *   commit          src/zeroskip-record.c:188-273 -- but with the WRITER's
 *                   long-commit trailer (src/zeroskip-file.c:266-302); the
 *                   reference verifier's long branch dereferences a length
 *   packed file     src/zeroskip-packed.c:70-131 (pointer section located from
 *                   the final commit at the end of the file), :278-339
 *   header CRC      src/zeroskip-header.c:105-170 (host-order fields)
 *   .zsdb CRC       src/zeroskip-dotzsdb.c:160-235 (host-order fields)
 * zscrc_zs_walk is the serial form of the walk, for images in host memory;
 * zscrc_device_walk (zscrc_walk.hip) walks a device-resident
 * image on the GPU with the same results, and zscrc_device_verify_image below
 * is zscrc_zs_verify_image for such an image.  Every byte of every commit
 * span and every trailer is checksummed and compared on the GPU.
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "../../include/zscrc.h"
#include "zscrc_internal.h"
#include "zscrc_records.h"

extern "C" int zscrc_internal_verify_commits(const void *d_image, uint64_t image_size, const uint64_t *d_off,
                                             const uint64_t *d_len, const uint32_t *d_seed, uint32_t *d_crc,
                                             uint32_t *d_status, size_t n, void *stream, int write,
                                             uint64_t max_len);

namespace {

constexpr uint64_t HDR = 40;
constexpr uint64_t SIGNATURE = 0x5a45524f534b4950ull; /* zeroskip-priv.h:49 */
enum {
    T_KEY = 1, T_VALUE = 2, T_COMMIT = 4, T_2ND = 8, T_FINAL = 16, T_LONG = 32, T_DELETED = 64,
    T_LONG_KEY = 33, T_LONG_VALUE = 34, T_LONG_COMMIT = 36, T_LONG_FINAL = 48,
    T_LONG_DELETED_ALIAS = 32, /* REC_TYPE_LONG_DELETED = LONG|LONG (zeroskip-priv.h:119) */
};

inline uint64_t be64(const uint8_t *p)
{
    uint64_t v;
    memcpy(&v, p, 8);
    return __builtin_bswap64(v);
}
inline uint32_t be32(const uint8_t *p)
{
    uint32_t v;
    memcpy(&v, p, 4);
    return __builtin_bswap32(v);
}
inline uint64_t rup8(uint64_t n) { return (n + 7) & ~7ull; }

/* Where the record parsers read the image from: host memory, or (the packed
 * file's few words, zscrc_device_verify_image) device memory one word a copy. */
struct HostImage {
    const uint8_t *img;
    uint64_t word(uint64_t off) const { return be64(img + off); }
};
struct DeviceImage {
    const uint8_t *d_img;
    hipStream_t stream;
    mutable bool failed = false;
    uint64_t word(uint64_t off) const
    {
        uint8_t b[8] = {};
        if (hipMemcpyAsync(b, d_img + off, 8, hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess)
            failed = true;
        return be64(b);
    }
};

/* commit_at and packed_spans over either reader: zscrc_records.h (the device
 * record lister reads a packed file's words through them in a kernel). */
using zsrec::commit_at;
using zsrec::packed_spans;

/* The commits' statuses of a device-resident image into the report. */
int verify_spans(const void *d_image, uint64_t size, const uint64_t *d_off, const uint64_t *d_len, size_t n,
                 uint64_t max_len, uint32_t *d_crc, uint32_t *d_st, hipStream_t stream, zscrc_zs_report *rep)
{
    int rc = zscrc_device_verify_commits_bounded(d_image, size, d_off, d_len, nullptr, n, max_len, d_crc, d_st,
                                                 stream);
    if (rc)
        return rc;
    uint32_t *st = static_cast<uint32_t *>(malloc(n * 4));
    if (!st)
        return ZSCRC_ENOMEM;
    if (hipMemcpyAsync(st, d_st, n * 4, hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess) {
        rc = ZSCRC_EHIP;
    } else {
        for (size_t i = 0; i < n; ++i) {
            if (st[i] != 1) {
                if (rep->n_bad == 0)
                    rep->first_bad = i;
                rep->n_bad++;
            }
        }
    }
    free(st);
    return rc;
}

} /* namespace */

extern "C" {

int zscrc_zs_walk(const void *image, uint64_t size, uint64_t *span_off, uint64_t *span_len, size_t cap,
                  size_t *n_commits, uint64_t *end_off)
{
    const uint8_t *img = static_cast<const uint8_t *>(image);
    size_t n = 0;
    uint64_t off = HDR;
    int rc = ZSCRC_ZS_END;
    if (!img || size < HDR)
        return ZSCRC_EINVAL;
    /* Every length word comes from the file, which may be corrupt: each step
     * is checked against the bytes left (`room`, never an add that can wrap),
     * so the next offset is always past the current one and inside the image
     * or the walk stops with TRUNCATED. */
    while (off < size) {
        const uint64_t room = size - off;
        if (room < 8) {
            rc = ZSCRC_ZS_TRUNCATED;
            break;
        }
        const uint64_t w = be64(img + off);
        const unsigned t = (unsigned)(w >> 56);
        if (t == T_KEY || t == T_LONG_KEY) {
            uint64_t voff;
            if (t == T_KEY) {
                voff = w & 0xFFFFFFFFull;
            } else {
                if (room < 24) {
                    rc = ZSCRC_ZS_TRUNCATED;
                    break;
                }
                voff = be64(img + off + 16);
            }
            /* the value record (16-byte header) starts voff bytes on */
            if (voff == 0 || voff > room || room - voff < 16) {
                rc = ZSCRC_ZS_TRUNCATED;
                break;
            }
            const uint64_t v = off + voff;
            const uint64_t vw = be64(img + v);
            const uint64_t vlen = (vw >> 56) == T_VALUE ? ((vw >> 32) & 0xFFFFFF) : be64(img + v + 8);
            const uint64_t vroom = size - v - 16;
            if (vlen > vroom || rup8(vlen) > vroom) { /* vlen <= vroom: rup8 cannot wrap */
                rc = ZSCRC_ZS_TRUNCATED;
                break;
            }
            off = v + 16 + rup8(vlen);
        } else if (t == T_DELETED || t == T_LONG_DELETED_ALIAS) {
            if (room < 24) {
                rc = ZSCRC_ZS_TRUNCATED;
                break;
            }
            const uint64_t klen = t == T_DELETED ? ((w >> 40) & 0xFFFF) : be64(img + off + 8);
            if (klen > room - 24 || rup8(klen) > room - 24) {
                rc = ZSCRC_ZS_TRUNCATED;
                break;
            }
            off += 24 + rup8(klen);
        } else if (t == T_COMMIT || t == T_LONG_COMMIT) {
            uint64_t sl, rl;
            if (!commit_at(HostImage{img}, size, off, &sl, &rl)) {
                rc = ZSCRC_ZS_TRUNCATED;
                break;
            }
            if (n < cap) {
                span_off[n] = off - sl;
                span_len[n] = sl;
            }
            ++n;
            off += rl;
        } else {
            rc = ZSCRC_ZS_STOPPED; /* FINAL / 2ND_HALF / UNUSED / VALUE: not advanced over */
            break;
        }
    }
    if (n_commits)
        *n_commits = n;
    if (end_off)
        *end_off = off;
    return n > cap ? ZSCRC_ZS_OVERFLOW : rc;
}

int zscrc_zs_packed_spans(const void *image, uint64_t size, uint64_t span_off[2], uint64_t span_len[2])
{
    if (!image)
        return ZSCRC_EINVAL;
    return packed_spans(HostImage{static_cast<const uint8_t *>(image)}, size, span_off, span_len);
}

int zscrc_zs_header_crc(const void *image, uint64_t size, uint32_t *stored, uint32_t *computed)
{
    const uint8_t *img = static_cast<const uint8_t *>(image);
    if (!img || size < HDR)
        return ZSCRC_EINVAL;
    uint64_t sig;
    memcpy(&sig, img, 8); /* native byte order (zeroskip-header.c:48) */
    const uint32_t version = be32(img + 8), sidx = be32(img + 28), eidx = be32(img + 32);
    uint32_t c = crc32c_hw(0, 0, 0);
    c = crc32c_hw(c, &sig, 8);
    c = crc32c_hw(c, &version, 4);
    c = crc32c_hw(c, img + 12, 16);
    c = crc32c_hw(c, &sidx, 4);
    c = crc32c_hw(c, &eidx, 4);
    *computed = c;
    *stored = be32(img + 36);
    return sig == SIGNATURE ? ZSCRC_OK : ZSCRC_ZS_BADSIG;
}

int zscrc_zs_dotzsdb_crc(const void *image, uint64_t size, uint32_t *stored, uint32_t *computed)
{
    /* struct dotzsdb (zeroskip-priv.h:83-91, packed): signature u64 (native),
     * offset u64 (BE), uuidstr[37], curidx u32 (BE), crc u32 (BE) = 61 bytes */
    const uint8_t *img = static_cast<const uint8_t *>(image);
    if (!img || size < 61)
        return ZSCRC_EINVAL;
    uint64_t sig;
    memcpy(&sig, img, 8);
    const uint64_t offset = be64(img + 8);
    const uint32_t curidx = be32(img + 53);
    uint32_t c = crc32c_hw(0, 0, 0);
    c = crc32c_hw(c, &sig, 8);
    c = crc32c_hw(c, &offset, 8);
    c = crc32c_hw(c, img + 16, 37);
    c = crc32c_hw(c, &curidx, 4);
    *computed = c;
    *stored = be32(img + 57);
    return sig == SIGNATURE ? ZSCRC_OK : ZSCRC_ZS_BADSIG;
}

int zscrc_device_verify_commits(const void *d_image, uint64_t image_size, const uint64_t *d_span_off,
                                const uint64_t *d_span_len, size_t n, uint32_t *d_crc, uint32_t *d_status,
                                void *stream)
{
    return zscrc_internal_verify_commits(d_image, image_size, d_span_off, d_span_len, nullptr, d_crc, d_status, n,
                                         stream, 0, ZSCRC_LEN_UNBOUNDED);
}

int zscrc_device_verify_commits_seeded(const void *d_image, uint64_t image_size, const uint64_t *d_span_off,
                                       const uint64_t *d_span_len, const uint32_t *d_seed, size_t n,
                                       uint32_t *d_crc, uint32_t *d_status, void *stream)
{
    return zscrc_internal_verify_commits(d_image, image_size, d_span_off, d_span_len, d_seed, d_crc, d_status, n,
                                         stream, 0, ZSCRC_LEN_UNBOUNDED);
}

int zscrc_device_verify_commits_bounded(const void *d_image, uint64_t image_size, const uint64_t *d_span_off,
                                        const uint64_t *d_span_len, const uint32_t *d_seed, size_t n,
                                        uint64_t max_len, uint32_t *d_crc, uint32_t *d_status, void *stream)
{
    return zscrc_internal_verify_commits(d_image, image_size, d_span_off, d_span_len, d_seed, d_crc, d_status, n,
                                         stream, 0, max_len);
}

int zscrc_device_write_commits_bounded(void *d_image, uint64_t image_size, const uint64_t *d_span_off,
                                       const uint64_t *d_span_len, size_t n, uint64_t max_len, uint32_t *d_crc,
                                       uint32_t *d_status, void *stream)
{
    return zscrc_internal_verify_commits(d_image, image_size, d_span_off, d_span_len, nullptr, d_crc, d_status, n,
                                         stream, 1, max_len);
}

int zscrc_device_commit_crcs_bounded(const void *d_image, uint64_t image_size, const uint64_t *d_span_off,
                                     const uint64_t *d_span_len, size_t n, uint64_t max_len, uint32_t *d_crc,
                                     uint32_t *d_status, void *stream)
{
    return zscrc_internal_verify_commits(d_image, image_size, d_span_off, d_span_len, nullptr, d_crc, d_status, n,
                                         stream, 2, max_len);
}

int zscrc_device_write_commits(void *d_image, uint64_t image_size, const uint64_t *d_span_off,
                               const uint64_t *d_span_len, size_t n, uint32_t *d_crc, uint32_t *d_status,
                               void *stream)
{
    return zscrc_internal_verify_commits(d_image, image_size, d_span_off, d_span_len, nullptr, d_crc, d_status, n,
                                         stream, 1, ZSCRC_LEN_UNBOUNDED);
}

int zscrc_zs_verify_image(const void *image, uint64_t size, int kind, zscrc_zs_report *rep)
{
    if (!image || !rep)
        return ZSCRC_EINVAL;
    memset(rep, 0, sizeof *rep);
    rep->header_rc = zscrc_zs_header_crc(image, size, &rep->header_stored, &rep->header_computed);
    uint64_t *off = nullptr, *len = nullptr;
    size_t n = 0;
    int rc;
    if (kind == ZSCRC_ZS_PACKED) {
        off = static_cast<uint64_t *>(malloc(2 * sizeof(uint64_t)));
        len = static_cast<uint64_t *>(malloc(2 * sizeof(uint64_t)));
        if (!off || !len) {
            free(off);
            free(len);
            return ZSCRC_ENOMEM;
        }
        rc = zscrc_zs_packed_spans(image, size, off, len);
        n = rc == ZSCRC_OK ? 2 : 0;
        rep->walk_rc = rc;
        rep->end_off = size;
    } else {
        /* a commit needs >= 8 bytes of file: bound the descriptor count */
        const size_t cap = (size_t)(size / 8) + 1;
        off = static_cast<uint64_t *>(malloc(cap * sizeof(uint64_t)));
        len = static_cast<uint64_t *>(malloc(cap * sizeof(uint64_t)));
        if (!off || !len) {
            free(off);
            free(len);
            return ZSCRC_ENOMEM;
        }
        rep->walk_rc = zscrc_zs_walk(image, size, off, len, cap, &n, &rep->end_off);
    }
    rep->n_commits = n;
    rc = ZSCRC_OK;
    if (n) {
        /* freed at the end of this block: the image, then the descriptors */
        zs::ScopedBuf<zs::Device> dmeta, dimg_buf;
        hipError_t e = zs::reserve_hip(dimg_buf, size);
        if (e == hipSuccess)
            e = zs::reserve_hip(dmeta, n * 24);
        void *const dimg = dimg_buf.as<void>();
        uint64_t *doff = dmeta.as<uint64_t>();
        uint64_t *dlen = doff + n;
        uint32_t *dcrc = reinterpret_cast<uint32_t *>(dlen + n);
        uint32_t *dst = dcrc + n;
        if (e == hipSuccess)
            e = hipMemcpy(dimg, image, size, hipMemcpyHostToDevice);
        if (e == hipSuccess)
            e = hipMemcpy(doff, off, n * 8, hipMemcpyHostToDevice);
        if (e == hipSuccess)
            e = hipMemcpy(dlen, len, n * 8, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            rc = ZSCRC_EHIP;
        } else {
            uint64_t max_len = 0;
            for (size_t i = 0; i < n; ++i)
                max_len = len[i] > max_len ? len[i] : max_len;
            rc = verify_spans(dimg, size, doff, dlen, n, max_len, dcrc, dst, nullptr, rep);
        }
    }
    free(off);
    free(len);
    return rc;
}

int zscrc_device_verify_image(const void *d_image, uint64_t image_size, int kind, zscrc_zs_report *rep, void *stream)
{
    if (!d_image || !rep)
        return ZSCRC_EINVAL;
    memset(rep, 0, sizeof *rep);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint8_t *dimg = static_cast<const uint8_t *>(d_image);
    uint8_t hdr[HDR];
    if (image_size >= HDR &&
        (hipMemcpyAsync(hdr, dimg, HDR, hipMemcpyDeviceToHost, s) != hipSuccess ||
         hipStreamSynchronize(s) != hipSuccess))
        return ZSCRC_EHIP;
    rep->header_rc = zscrc_zs_header_crc(hdr, image_size >= HDR ? HDR : image_size, &rep->header_stored,
                                         &rep->header_computed);
    /* device block of `cap` commits: offsets, lengths, CRCs, statuses (24
     * bytes a commit), then the walk's result words */
    zs::ScopedBuf<zs::Device> dmeta;
    size_t n = 0, cap = 2;
    uint64_t max_len = 0;
    int rc = ZSCRC_OK;
    auto block = [&dmeta](size_t c) { return dmeta.reserve(c * 24 + ZSCRC_WALK_RES_WORDS * 8); };
    if (kind == ZSCRC_ZS_PACKED) {
        uint64_t sp[4]; /* two offsets, two lengths */
        uint64_t so[2], sl[2];
        const DeviceImage im{dimg, s};
        rep->walk_rc = packed_spans(im, image_size, so, sl);
        rep->end_off = image_size;
        if (im.failed)
            return ZSCRC_EHIP;
        if (rep->walk_rc == ZSCRC_OK) {
            n = 2;
            sp[0] = so[0], sp[1] = so[1], sp[2] = sl[0], sp[3] = sl[1];
            max_len = sl[0] > sl[1] ? sl[0] : sl[1];
            rc = block(cap);
            if (!rc && (hipMemcpyAsync(dmeta.as<void>(), sp, sizeof sp, hipMemcpyHostToDevice, s) != hipSuccess ||
                        hipStreamSynchronize(s) != hipSuccess))
                rc = ZSCRC_EHIP;
        }
    } else if (image_size < HDR) {
        rep->walk_rc = ZSCRC_EINVAL; /* as zscrc_zs_walk */
    } else {
        /* most images hold far fewer commits than the bound size / 8 + 1: a
         * first walk with room for one commit per 64 bytes, and only if that
         * overflows a second one with room for the count the first one found */
        uint64_t res[ZSCRC_WALK_RES_WORDS] = {};
        cap = (size_t)(image_size / 64) + 1;
        for (int pass = 0; pass < 2; ++pass) {
            rc = block(cap); /* the second pass frees the first one's, then allocates */
            if (rc)
                break;
            uint64_t *doff = dmeta.as<uint64_t>(), *dres = doff + 3 * cap;
            rc = zscrc_device_walk(d_image, image_size, doff, doff + cap, cap, dres, nullptr, nullptr, 0, s);
            if (!rc && (hipMemcpyAsync(res, dres, sizeof res, hipMemcpyDeviceToHost, s) != hipSuccess ||
                        hipStreamSynchronize(s) != hipSuccess))
                rc = ZSCRC_EHIP;
            if (rc || res[1] <= cap)
                break;
            cap = (size_t)res[1];
        }
        if (!rc) {
            rep->walk_rc = (int)res[0];
            n = (size_t)res[1];
            rep->end_off = res[2];
            max_len = res[3];
        }
    }
    rep->n_commits = n;
    if (!rc && n) {
        uint64_t *doff = dmeta.as<uint64_t>();
        uint32_t *dcrc = reinterpret_cast<uint32_t *>(doff + 2 * cap);
        rc = verify_spans(d_image, image_size, doff, doff + cap, n, max_len, dcrc, dcrc + cap, s, rep);
    }
    return rc;
}

} /* extern "C" */
