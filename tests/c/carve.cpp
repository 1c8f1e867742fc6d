/*
 * carve.cpp -- zs::Carve, the scratch layout of the device stages, on the CPU
 * (tests/test_carve.py).  Includes only zscrc_carve.h.  The way a stage does,
 * one function takes pieces of mixed types, counts and alignments out of a
 * Carve, zero-count pieces among them; it runs on a NULL base (the sizing
 * call) and on a buffer of exactly the bytes that run gave (the launch), at
 * several sets of counts.  Checked: both runs give the same bytes(); on a NULL
 * base every piece is NULL; on the buffer every piece is aligned as asked,
 * begins at or after the end of the piece before it, by less than its
 * alignment, and the last one ends at bytes().  Every piece is then written
 * end to end, so a sanitizer sees a piece that leaves the buffer.
 *
 *   carve          exit status 0 = all of the above holds
 *   carve overrun  as above, then one byte past bytes() is written: a run
 *                  under the address sanitizer must fail
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../zeroskip_amd/csrc/zscrc_carve.h"

struct Rec32 {
    uint64_t w[4];
};
struct Desc24 {
    const void *p;
    uint64_t a, b;
};

struct Piece {
    uint8_t *p;
    size_t bytes, align;
};

template <class T>
static void take(zs::Carve &c, std::vector<Piece> &out, size_t count, size_t align)
{
    T *p = c.take<T>(count, align);
    out.push_back(Piece{reinterpret_cast<uint8_t *>(p), count * sizeof(T), align});
}

/* The pieces of one call: words, descriptors, 8-byte arrays packed behind one
 * another, records, 4-byte and 1-byte arrays on 16-byte boundaries. */
static size_t carve(zs::Carve c, const size_t n[4], std::vector<Piece> &out)
{
    out.clear();
    take<unsigned long long>(c, out, 16, 16);
    take<Desc24>(c, out, n[0] + 1, 16);
    take<uint64_t>(c, out, n[1], alignof(uint64_t));
    take<uint64_t>(c, out, n[1] + 1, alignof(uint64_t));
    take<Rec32>(c, out, n[2], 16);
    take<uint32_t>(c, out, n[3], 16);
    take<uint8_t>(c, out, 0, 16);
    take<uint8_t>(c, out, n[2], 16);
    take<uint32_t>(c, out, n[0], 64);
    take<uint8_t>(c, out, n[3], 1);
    return c.bytes();
}

static int fail(const char *what, size_t a, size_t b)
{
    fprintf(stderr, "carve: %s (%zu, %zu)\n", what, a, b);
    return 1;
}

int main(int argc, char **argv)
{
    const bool overrun = argc == 2 && !strcmp(argv[1], "overrun");
    static const size_t sets[][4] = {{0, 0, 0, 0}, {1, 1, 1, 1},   {3, 5, 7, 11},        {1, 0, 3, 0},
                                     {0, 2, 0, 5}, {64, 1023, 1025, 4097}, {17, 1, 100000, 3}};
    std::vector<Piece> sized, real;
    size_t cases = 0;
    for (const auto &n : sets) {
        const size_t need = carve(zs::Carve(nullptr), n, sized);
        for (const Piece &p : sized)
            if (p.p)
                return fail("a piece of a NULL base is not NULL", cases, 0);
        /* exactly `need` bytes at a 64-byte boundary: the largest alignment asked */
        void *exact = nullptr;
        if (posix_memalign(&exact, 64, need))
            return fail("no memory", need, 0);
        uint8_t *buf = static_cast<uint8_t *>(exact);
        const size_t got = carve(zs::Carve(buf), n, real);
        if (got != need)
            return fail("bytes() of the two runs differ", need, got);
        if (real.size() != sized.size())
            return fail("piece counts differ", sized.size(), real.size());
        size_t end = 0;
        for (size_t i = 0; i < real.size(); ++i) {
            const Piece &p = real[i];
            const size_t at = (size_t)(p.p - buf);
            if (p.bytes != sized[i].bytes)
                return fail("piece sizes differ", i, p.bytes);
            if (reinterpret_cast<uintptr_t>(p.p) % p.align)
                return fail("a piece is not aligned as asked", i, at);
            if (at < end)
                return fail("a piece begins inside the one before it", i, at);
            if (at - end >= p.align)
                return fail("a gap of a whole alignment or more", i, at - end);
            memset(p.p, (int)(i + 1), p.bytes);
            end = at + p.bytes;
        }
        if (end != need)
            return fail("the last piece does not end at bytes()", end, need);
        /* no piece overwrote another one */
        for (size_t i = 0; i < real.size(); ++i)
            for (size_t b = 0; b < real[i].bytes; ++b)
                if (real[i].p[b] != (uint8_t)(i + 1))
                    return fail("two pieces share a byte", i, b);
        if (overrun) {
            volatile uint8_t *past = buf + need;
            *past = 1;
        }
        free(buf);
        ++cases;
    }
    printf("ok %zu cases\n", cases);
    return 0;
}
