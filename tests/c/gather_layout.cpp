/*
 * gather_layout.cpp -- the value gather's shared arithmetic on the CPU
 * (tests/test_gather_layout.py).  Includes only the header the kernels of
 * zscrc_gather.hip share with the host, reads a case file
 *
 *   u64 src_len, nq, shift, want_len;
 *   src[src_len]; items[nq] (4 x u64); want[want_len] (the gathered bytes)
 *
 * and gathers the way the library does: every item classified and a value
 * checked against the source, the saturating prefix of the lengths, then the
 * output built through build8 twice -- eight bytes at a time with the item
 * carried along (the host twin's loop), and one 16-byte word at a time with the
 * word's first item found by find_rec over the starts (a kernel thread's work),
 * the words taken from the last one down so that nothing is carried between
 * them.  The source lies at an address = shift mod 8 in an allocation that
 * ends with its last 8-byte granule, and the outputs have exactly total bytes,
 * so a sanitizer sees any read outside the aligned words that hold value bytes
 * and any write outside the output.
 * Exit status 0 = both outputs equal the expected bytes.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../zeroskip_amd/csrc/zscrc_gather_layout.h"

using namespace zsgather;

struct Item {
    uint64_t w0, w1, val_off, val_len;
};

static int fail(const char *what, uint64_t a, uint64_t b, uint64_t c)
{
    fprintf(stderr, "gather_layout: %s (%llu, %llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b,
            (unsigned long long)c);
    return 1;
}

int main(int argc, char **argv)
{
    if (argc != 2)
        return fail("usage: gather_layout CASEFILE", 0, 0, 0);
    FILE *f = fopen(argv[1], "rb");
    uint64_t hd[4];
    if (!f || fread(hd, 8, 4, f) != 4)
        return fail("cannot read the case", 0, 0, 0);
    const uint64_t src_len = hd[0], nq = hd[1], shift = hd[2] & 7, want_len = hd[3];
    const uint64_t gran = (shift + src_len + 7) & ~7ull;
    uint8_t *buf = static_cast<uint8_t *>(malloc(gran ? gran : 8));
    uint8_t *src = buf + shift;
    std::vector<Item> items(nq);
    std::vector<uint8_t> want(want_len);
    if ((src_len && fread(src, 1, src_len, f) != src_len) || (nq && fread(items.data(), 32, nq, f) != nq) ||
        (want_len && fread(want.data(), 1, want_len, f) != want_len))
        return fail("short case file", src_len, nq, want_len);
    fclose(f);

    /* size: the kinds, the check, the starts */
    std::vector<uint64_t> offs(nq + 1);
    uint64_t total = 0, count[KINDS] = {0, 0, 0, 0};
    for (uint64_t i = 0; i < nq; ++i) {
        const Kind k = kind_of(items[i].w0, items[i].val_off);
        if (k == VALUE && !value_ok(items[i].val_off, items[i].val_len, src_len))
            return fail("value outside the source", i, items[i].val_off, items[i].val_len);
        ++count[k];
        offs[i] = total;
        total = sum_len(total, len_of(k, items[i].val_len));
    }
    offs[nq] = total;
    if (count[VALUE] + count[DELETED] + count[NOT_FOUND] + count[BAD_QUERY] != nq)
        return fail("the kinds do not add up", nq, count[VALUE], count[DELETED]);
    if (total != want_len)
        return fail("total differs from the expected length", total, want_len, 0);

    const uint64_t *o = offs.data();
    const Item *it = items.data();
    const auto val_off = [it](uint64_t i) { return it[i].val_off; };
    /* the host twin's loop */
    uint8_t *a = static_cast<uint8_t *>(malloc(total ? total : 1));
    uint64_t j = 0;
    for (uint64_t p = 0; p < total; p += 8) {
        const uint32_t n = total - p < 8 ? (uint32_t)(total - p) : 8;
        const uint64_t v = build8(src, o, val_off, j, p, n);
        if (j >= nq)
            return fail("the carried item left the list", j, p, nq);
        memcpy(a + p, &v, n);
    }
    /* a kernel thread's word, the last word first */
    uint8_t *b = static_cast<uint8_t *>(malloc(total ? total : 1));
    for (uint64_t w = (total + 15) / 16; w-- > 0;) {
        const uint64_t p = 16 * w;
        const uint32_t n = total - p < 16 ? (uint32_t)(total - p) : 16;
        uint64_t k = zspack::find_rec(o, nq, p);
        if (o[k] > p || o[k + 1] <= p)
            return fail("find_rec did not land on the item that holds the byte", k, p, o[k]);
        const uint64_t v0 = build8(src, o, val_off, k, p, n < 8 ? n : 8);
        const uint64_t v1 = n > 8 ? build8(src, o, val_off, k, p + 8, n - 8) : 0;
        memcpy(b + p, &v0, n < 8 ? n : 8);
        if (n > 8)
            memcpy(b + p + 8, &v1, n - 8);
    }
    for (uint64_t p = 0; p < total; ++p)
        if (a[p] != want[p] || b[p] != want[p])
            return fail("output byte differs at, carried, searched", p, a[p], b[p]);
    free(a);
    free(b);
    free(buf);
    printf("ok %llu items %llu bytes\n", (unsigned long long)nq, (unsigned long long)total);
    return 0;
}
