/*
 * zscrc_log.cpp -- zscrc_zs_log, the host twin of the device log writer
 * (zscrc_device_log, zscrc_devlog.hip): the same record list, transaction
 * table and options in host memory give the same bytes and the same result
 * words.  It is built from the layout functions the kernels call
 * (zscrc_log_layout.h, zscrc_pack_layout.h) in the kernels' order -- the two
 * prefix sums, the spans, the starts, every record word by word through
 * piece_at -- and the host CRC; what it does not share with the device is the
 * load of source bytes (a memcpy of the bytes themselves instead of gather8's
 * aligned words) and crc32c_hw over each span.
 */
#include <cstring>
#include <new>
#include <vector>

#include "../../include/zscrc.h"
#include "zscrc_log_layout.h"

namespace {

using namespace zspack;

inline void put_word(uint8_t *out, uint64_t off, uint64_t w) { memcpy(out + off, &w, 8); }

/* The record at file offset st, word by word. */
void put_record(uint8_t *out, uint64_t st, const uint8_t *src, const zscrc_zs_record &r)
{
    const uint64_t len = rec_len(r);
    for (uint64_t rel = 0; rel < len; rel += 8) {
        const Piece pc = piece_at(r, rel);
        uint64_t w = pc.word;
        if (pc.n) {
            w = 0;
            memcpy(&w, src + pc.src_off, pc.n);
        }
        put_word(out, st + rel, w);
    }
}

/* The commit record behind a span; returns its stored CRC. */
uint32_t put_commit(uint8_t *out, uint64_t off, uint32_t span_crc, uint64_t span_len)
{
    uint64_t w[3];
    uint32_t stored;
    const int k = commit_words(span_crc, span_len, false, w, &stored);
    for (int i = 0; i < k; ++i)
        put_word(out, off + 8 * i, w[i]);
    return stored;
}

int log_host(const uint8_t *src, uint64_t src_size, const zscrc_zs_record *recs, uint64_t n, const uint64_t *tx_end,
             uint64_t ntx, const uint8_t *uuid, uint32_t startidx, uint32_t endidx, uint8_t *out, uint64_t out_cap,
             uint64_t at, zscrc_zs_record *new_recs, uint64_t *span_off, uint64_t *span_len, uint64_t *res,
             uint32_t prev_crc, bool finalise)
{
    using namespace zslog;
    /* P[i] and D[i] */
    std::vector<uint64_t> P(n + 1), C(ntx + 1), first(ntx), slen(ntx);
    std::vector<uint32_t> D(n);
    uint64_t bad = U64_MAX, top = 0;
    P[0] = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const bool b = rec_bad(recs[i], src_size);
        if (b && bad == U64_MAX)
            bad = i;
        P[i + 1] = sat_add(P[i], b ? 0 : rec_len(recs[i]));
        top = mark_max(top, b ? 0 : del_mark(recs[i], i));
        D[i] = (uint32_t)top;
    }
    /* the table, the spans, C[t] */
    uint64_t badtx = ntx || !n ? U64_MAX : 0;
    C[0] = 0;
    for (uint64_t t = 0; t < ntx; ++t) {
        const uint64_t b = tx_begin(tx_end, t), e = tx_stop(tx_end, t);
        uint64_t clen = 0;
        if (!tx_ok(b, e, t, ntx, n)) {
            if (badtx == U64_MAX)
                badtx = t;
        } else {
            const uint64_t s = span_first(b, e, e > b ? D[e - 1] : 0);
            first[t] = P[s];
            slen[t] = span_bytes(P[s], P[e]);
            clen = commit_len(slen[t]);
        }
        C[t + 1] = C[t] + clen;
    }
    const Totals tot = totals(at, P[n], C[ntx], ntx, finalise);
    const bool inval = bad != U64_MAX || badtx != U64_MAX;
    const uint64_t code = inval ? (uint64_t)(int64_t)ZSCRC_EINVAL : tot.end > out_cap ? (uint64_t)ZSCRC_ZS_OVERFLOW : 0;
    res[0] = code;
    res[1] = inval ? bad : n;
    res[2] = inval ? badtx : tot.end;
    res[3] = inval ? 0 : tot.written;
    res[4] = inval ? 0 : tot.commits;
    res[5] = code ? 0 : tot.long_commits;
    res[6] = res[7] = 0;
    if (code)
        return ZSCRC_OK;

    const uint64_t base = base_of(at);
    uint32_t reg = prev_crc, stored = 0;
    for (uint64_t t = 0; t < ntx; ++t) {
        const uint64_t b = tx_begin(tx_end, t), e = tx_stop(tx_end, t);
        for (uint64_t i = b; i < e; ++i) {
            const uint64_t st = placed(base, P[i], C[t]);
            put_record(out, st, src, recs[i]);
            if (new_recs)
                new_recs[i] = listed(recs[i], st);
        }
        const uint64_t off = placed(base, first[t], C[t]);
        reg = crc32c_hw(0, out + off, slen[t]);
        stored = put_commit(out, off + slen[t], reg, slen[t]);
        if (span_off) {
            span_off[t] = off;
            span_len[t] = slen[t];
        }
    }
    if (finalise) {
        /* no bytes, hashed from the register the last span left */
        stored = put_commit(out, tot.body_end, reg, 0);
        if (span_off) {
            span_off[ntx] = tot.body_end;
            span_len[ntx] = 0;
        }
    }
    if (at == 0) {
        const Header h = header_words(uuid, startidx, endidx);
        for (int i = 0; i < 5; ++i)
            put_word(out, 8 * i, h.w[i]);
    }
    res[6] = reg;
    res[7] = stored;
    return ZSCRC_OK;
}

} /* namespace */

extern "C" int zscrc_zs_log(const void *src, uint64_t src_size, const struct zscrc_zs_record *recs, size_t n,
                            const uint64_t *tx_end, size_t n_tx, const uint8_t uuid[16], uint32_t startidx,
                            uint32_t endidx, void *out, uint64_t out_cap, uint64_t at,
                            struct zscrc_zs_record *new_recs, uint64_t *span_off, uint64_t *span_len,
                            uint64_t res[ZSCRC_LOG_RES_WORDS], const zscrc_log_opts *opts, unsigned flags)
{
    const uint64_t tile = opts ? opts->tile_bytes : 0;
    const uintptr_t so = reinterpret_cast<uintptr_t>(src), oo = reinterpret_cast<uintptr_t>(out);
    if (!res || (at == 0 && !uuid) || (n && !recs) || (n_tx && !tx_end) || (!span_off != !span_len) ||
        (flags & ~ZSCRC_LOG_FINALISE) || (tile && (tile & (tile - 1) || tile < 64 || tile > 65536)) ||
        !zslog::counts_ok(n, n_tx, src_size) || !zslog::at_ok(at) || (out_cap && at > out_cap) ||
        (!out && out_cap) || (!src && src_size) || out_cap > UINTPTR_MAX - oo || src_size > UINTPTR_MAX - so)
        return ZSCRC_EINVAL;
    /* only the bytes the call may write must not overlap the source */
    if (out_cap > at && src_size && oo + at < so + src_size && so < oo + out_cap)
        return ZSCRC_EINVAL;
    try {
        return log_host(static_cast<const uint8_t *>(src), src_size, recs, n, tx_end, tx_end ? n_tx : n, uuid, startidx,
                        endidx, static_cast<uint8_t *>(out), out_cap, at, new_recs, span_off, span_len, res,
                        opts ? opts->prev_crc : 0, (flags & ZSCRC_LOG_FINALISE) != 0);
    } catch (const std::bad_alloc &) {
        return ZSCRC_ENOMEM;
    }
}
