/*
 * pack_layout.cpp -- the device packer's layout arithmetic on the CPU
 * (tests/test_pack_layout.py).  Includes only the header the kernels of
 * zscrc_devpack.hip share with the host, reads a case file
 *
 *   u64 src_len, n, file_len, shift, startidx, endidx; uuid[16];
 *   src[src_len]; recs[n] (4 x u64); file[file_len] (the expected packed file)
 *
 * and rebuilds the file the way the kernels do: record lengths and starts,
 * the layout, then for each tile size the records region tile by tile and word
 * by word (find_rec, piece_at, gather8), the pointers, the two commit records
 * from bitwise span CRCs, the header.  The source lies at an address = shift
 * mod 8 in an allocation that ends with its last 8-byte granule, so a
 * sanitizer sees any read outside the aligned words that hold source bytes.
 * Exit status 0 = every byte equal at every tile size.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../zeroskip_amd/csrc/zscrc_pack_layout.h"

using namespace zspack;

static int fail(const char *what, uint64_t a, uint64_t b, uint64_t c)
{
    fprintf(stderr, "pack_layout: %s (%llu, %llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b,
            (unsigned long long)c);
    return 1;
}

static uint32_t crc_span(const uint8_t *p, uint64_t n)
{
    uint32_t c = 0;
    for (uint64_t i = 0; i < n; ++i)
        c = crc_bytes(c, p[i], 1);
    return c;
}

int main(int argc, char **argv)
{
    if (argc != 2)
        return fail("usage: pack_layout CASEFILE", 0, 0, 0);
    FILE *f = fopen(argv[1], "rb");
    uint64_t hd[6];
    uint8_t uuid[16];
    if (!f || fread(hd, 8, 6, f) != 6 || fread(uuid, 1, 16, f) != 16)
        return fail("cannot read the case", 0, 0, 0);
    const uint64_t src_len = hd[0], n = hd[1], file_len = hd[2], shift = hd[3] & 7;
    const uint64_t gran = (shift + src_len + 7) & ~7ull;
    uint8_t *buf = static_cast<uint8_t *>(malloc(gran ? gran : 8));
    uint8_t *src = buf + shift;
    std::vector<zscrc_zs_record> recs(n);
    std::vector<uint8_t> want(file_len);
    if ((src_len && fread(src, 1, src_len, f) != src_len) || (n && fread(recs.data(), 32, n, f) != n) ||
        (file_len && fread(want.data(), 1, file_len, f) != file_len))
        return fail("short case file", src_len, n, file_len);
    fclose(f);

    /* lengths, starts, layout */
    std::vector<uint64_t> start(n + 1);
    uint64_t R = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (!rec_ok(recs[i], src_len))
            return fail("record outside the source", i, recs[i].key_off, recs[i].key_len);
        start[i] = R;
        R = sat_add(R, rec_len(recs[i]));
    }
    start[n] = R;
    const Layout l = layout(n, R);
    if (l.file_bytes != file_len)
        return fail("file size", l.file_bytes, file_len, R);

    const uint64_t tiles[4] = {64, 128, 4096, 65536};
    for (uint64_t T : tiles) {
        /* 8-byte words, so that the output is built the way the kernel stores it */
        std::vector<uint64_t> out(file_len / 8 + 1, 0xA5A5A5A5A5A5A5A5ull);
        uint64_t written = 0;
        if (R) {
            const uint64_t nt = tile_count(T, R);
            uint64_t lo, hi;
            tile_range(0, T, R, &lo, &hi);
            uint64_t rec0 = find_rec(start, n, lo);
            for (uint64_t t = 0; t < nt; ++t) {
                tile_range(t, T, R, &lo, &hi);
                if (lo >= hi || hi > R || (t + 1 == nt) != (hi == R))
                    return fail("tile range", t, lo, hi);
                if (rec0 != find_rec(start, n, lo))
                    return fail("running first record", t, rec0, find_rec(start, n, lo));
                const uint64_t *s = start.data() + rec0;
                uint64_t m = 0;
                while (s[m] < hi)
                    ++m;
                if (m == 0 || m > T / 24 + 2)
                    return fail("records of a tile", t, m, T);
                for (uint64_t p = lo; p < hi; p += 8) {
                    if ((HDR + p) / T != t)
                        return fail("word outside its tile", t, p, T);
                    const uint64_t j = find_rec(s, m, p);
                    const Piece pc = piece_at(recs[rec0 + j], p - s[j]);
                    out[(HDR + p) / 8] = pc.n ? gather8(src + pc.src_off, pc.n) : pc.word;
                    ++written;
                }
                rec0 += s[m] == hi ? m : m - 1;
            }
        }
        if (written != R / 8)
            return fail("words written", written, R / 8, T);
        /* pointers and count, commits, header */
        out[l.ptr_off / 8] = mem_be64(n);
        for (uint64_t i = 0; i < n; ++i)
            out[l.ptr_off / 8 + 1 + i] = mem_be64(HDR + start[i]);
        const uint8_t *ob = reinterpret_cast<const uint8_t *>(out.data());
        uint64_t w[3];
        uint32_t stored;
        int k = commit_words(crc_span(ob + HDR, R), R, false, w, &stored);
        if ((uint64_t)k * 8 != commit_len(R))
            return fail("region commit length", k, R, 0);
        for (int i = 0; i < k; ++i)
            out[(HDR + R) / 8 + i] = w[i];
        k = commit_words(crc_span(ob + l.ptr_off, l.ptr_bytes), l.ptr_bytes, true, w, &stored);
        for (int i = 0; i < k; ++i)
            out[(l.ptr_off + l.ptr_bytes) / 8 + i] = w[i];
        const Header h = header_words(uuid, (uint32_t)hd[4], (uint32_t)hd[5]);
        for (int i = 0; i < 5; ++i)
            out[i] = h.w[i];
        if (memcmp(ob, want.data(), file_len) != 0) {
            uint64_t at = 0;
            while (ob[at] == want[at])
                ++at;
            return fail("byte differs at, tile, file", at, T, file_len);
        }
        if (out[file_len / 8] != 0xA5A5A5A5A5A5A5A5ull)
            return fail("word past the file written", T, file_len, 0);
    }
    free(buf);
    printf("ok %llu records %llu bytes\n", (unsigned long long)n, (unsigned long long)file_len);
    return 0;
}
