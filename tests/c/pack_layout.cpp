/*
 * pack_layout.cpp -- the device packer's layout arithmetic on the CPU
 * (tests/test_pack_layout.py).  Includes only the headers the kernels of
 * zscrc_devpack.hip share with the host, reads a case file
 *
 *   u64 src_len, n, file_len, shift, startidx, endidx; uuid[16];
 *   src[src_len]; recs[n] (4 x u64); file[file_len] (the expected packed file)
 *
 * and rebuilds the file the way the kernels do: record lengths and starts,
 * the layout, then for each tile size the records region by the kernel's own
 * tile sweep (copy_tiles_sweep.h) at four grid sizes, the pointers, the two
 * commit records from bitwise span CRCs, the header.  The source lies at an
 * address = shift mod 8 in an allocation that ends with its last 8-byte
 * granule, so a sanitizer sees any read outside the aligned words that hold
 * source bytes.
 * Exit status 0 = every byte equal at every tile and grid size; the ok line
 * counts the stores of each kind.
 */
#include <cstdlib>
#include <cstring>

static const char *PROGRAM = "pack_layout";
#include "copy_tiles_sweep.h"

using namespace zspack;

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
    Stores stores{0, 0, 0};
    for (uint64_t T : tiles) {
        /* 8-byte words, so that the output is built the way the kernel stores it */
        std::vector<uint64_t> out(file_len / 8 + 1, CANARY);
        if (R && sweep<HDR, false>(src, recs, start, T, HDR, HDR + R, R / 8, out, stores))
            return 1;
        /* the sweep's tiles in file coordinates are zscrc_pack_layout.h's in region coordinates */
        for (uint64_t t = 0, lo, hi; R && t <= tile_count(T, R); ++t) {
            tile_range(t, T, R, &lo, &hi);
            if (t == tile_count(T, R) ? zstile::run_of(0, 1, T, HDR, HDR + R).t1 != t
                                      : zstile::tile_lo(t, T, HDR) != HDR + lo || zstile::tile_hi(t, T, HDR + R) != HDR + hi)
                return fail("tiles in file and in region coordinates", t, lo, hi);
        }
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
        if (out[file_len / 8] != CANARY)
            return fail("word past the file written", T, file_len, 0);
    }
    free(buf);
    printf("ok %llu records %llu bytes; stores: %llu of 16 bytes, %llu of a first half, %llu of a second half\n",
           (unsigned long long)n, (unsigned long long)file_len, (unsigned long long)stores.both,
           (unsigned long long)stores.first, (unsigned long long)stores.second);
    return 0;
}
