/*
 * devbuf.cpp -- zs::Buf, zs::ScopedBuf and zs::reserve_all, the owners of the
 * host library's device and pinned memory, on the CPU (tests/test_devbuf.py).
 * Includes only zscrc_buf.h.  The backend is malloc with a log: every
 * allocation and free with its size, the live allocations, and an order to
 * fail the k-th allocation from now.  Checked: when reserve() calls the
 * backend and when not, the order free-then-allocate, the bytes every site's
 * slack gives against the expression the site had before zs::Buf, the state
 * after a failed allocation, release() twice, swap(), the order in which ScopedBufs
 * leave a scope, and the group helper with a failure at every position.  The
 * buffers are written end to end, so a sanitizer sees one that is too small,
 * and nothing is live at exit (the leak sanitizer checks the same).
 *
 *   devbuf    exit status 0 and "ok <checks> checks, 0 live" = all of it holds
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "../../zeroskip_amd/csrc/zscrc_buf.h"

struct Call {
    bool alloc; /* else free */
    size_t bytes;
    void *p; /* NULL: the allocation that was told to fail */
};

struct Counting {
    static std::vector<Call> log;
    static std::map<void *, size_t> live;
    static size_t fail_in; /* the k-th allocation from now fails; 0 = none */
    static constexpr int CODE = 2; /* what the backend answers then (hipErrorOutOfMemory's value) */

    static int alloc(void **p, size_t n)
    {
        if (fail_in && --fail_in == 0) {
            log.push_back(Call{true, n, nullptr});
            return CODE;
        }
        *p = malloc(n);
        if (!*p)
            abort();
        memset(*p, 0xA5, n);
        live[*p] = n;
        log.push_back(Call{true, n, *p});
        return 0;
    }
    static void free(void *p)
    {
        if (!live.count(p))
            abort(); /* a free of what is not allocated */
        log.push_back(Call{false, live[p], p});
        live.erase(p);
        ::free(p);
    }
};
std::vector<Call> Counting::log;
std::map<void *, size_t> Counting::live;
size_t Counting::fail_in = 0;

using Buf = zs::Buf<Counting>;
using Scoped = zs::ScopedBuf<Counting>;

static_assert(std::is_trivially_destructible<Buf>::value, "a cached buffer frees nothing from a static destructor");
static_assert(!std::is_trivially_destructible<Scoped>::value, "a call's buffer is freed at the end of its scope");
static_assert(!std::is_copy_constructible<Buf>::value && !std::is_copy_assignable<Buf>::value &&
                  !std::is_move_constructible<Scoped>::value && !std::is_move_assignable<Scoped>::value,
              "one owner");
static_assert(std::is_default_constructible<Buf[4]>::value, "caches hold arrays of them");

static size_t g_checks = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        ++g_checks;                                                          \
        if (!(cond)) {                                                       \
            fprintf(stderr, "devbuf: line %d: %s\n", __LINE__, #cond);       \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

static size_t calls() { return Counting::log.size(); }
static const Call &last(size_t back = 0) { return Counting::log[calls() - 1 - back]; }

/* The slack of every site, beside the expression the site had before zs::Buf
 * (`old`: the bytes it allocated for a need of x; for the groups, per unit of
 * width).  need(x) is the first argument the site passes, slack(x) the second. */
struct Site {
    const char *name;
    size_t (*need)(size_t), (*slack)(size_t), (*old)(size_t);
};
static const Site sites[] = {
    /* zscrc_api.cpp grow():  size_t n = need + need / 4; */
    {"api grow", [](size_t x) { return x; }, [](size_t x) { return x / 4; }, [](size_t x) { return x + x / 4; }},
    /* zscrc_files.cpp grow_dev():  need += need / 8; */
    {"files grow_dev", [](size_t x) { return x; }, [](size_t x) { return x / 8; }, [](size_t x) { return x + x / 8; }},
    /* zscrc_fill.cpp ensure(), the ring:  hipMalloc(&b, chunk_bytes + 256) when ring_bytes < chunk_bytes + 256 */
    {"fill ring", [](size_t x) { return x + 256; }, [](size_t) { return (size_t)0; }, [](size_t x) { return x + 256; }},
    /* zscrc_fill.cpp ensure(), the pairs:  m = c + c / 4 + 64;  hipMalloc(&p, 28 * m + 64) when ring_commits < c */
    {"fill pairs", [](size_t c) { return 28 * c + 64; }, [](size_t c) { return 28 * (c / 4 + 64); },
     [](size_t c) { return 28 * (c + c / 4 + 64) + 64; }},
    /* zscrc_fill.cpp ensure(), the host arrays:  m = n + n / 4 + 1024;  8 * m and 4 * m bytes;
     * zscrc_files.cpp ensure_desc():  count += count / 4 + 1024;  8, 8 and 4 bytes x count */
    {"host arrays, descriptors", [](size_t n) { return n; }, [](size_t n) { return n / 4 + 1024; },
     [](size_t n) { return n + n / 4 + 1024; }},
    /* zscrc_scratch.cpp scratch_acquire(), stage_begin(), every buffer of a fixed size:  none */
    {"none", [](size_t x) { return x; }, [](size_t) { return (size_t)0; }, [](size_t x) { return x; }},
};

static void fill(const Buf &b)
{
    if (b.bytes())
        memset(b.as<uint8_t>(), 0x5A, b.bytes());
}

static void reserve_rules()
{
    Buf b;
    CHECK(b.bytes() == 0 && b.as<void>() == nullptr);
    CHECK(b.reserve(0) == ZSCRC_OK && calls() == 0); /* an empty buffer is large enough for nothing */
    CHECK(b.reserve(1000, 24) == ZSCRC_OK && calls() == 1 && last().alloc && last().bytes == 1024);
    CHECK(b.bytes() == 1024);
    fill(b);
    void *p = b.as<void>();
    for (size_t need : {0, 1, 1000, 1024}) /* up to the bytes it has, slack included: no call, same pointer */
        CHECK(b.reserve(need, 512) == ZSCRC_OK && calls() == 1 && b.as<void>() == p && b.bytes() == 1024);
    /* growth: the old bytes are freed, once, before the new ones are asked for */
    CHECK(b.reserve(1025, 7) == ZSCRC_OK && calls() == 3);
    CHECK(!last(1).alloc && last(1).p == p && last(1).bytes == 1024 && last().alloc && last().bytes == 1032);
    CHECK(b.bytes() == 1032 && Counting::live.size() == 1);
    fill(b);
    /* a failed allocation: freed first all the same, then empty, with the backend's code kept */
    Counting::fail_in = 1;
    CHECK(b.reserve(5000, 10) == ZSCRC_ENOMEM && calls() == 5 && !last(1).alloc && last().bytes == 5010);
    CHECK(b.as<void>() == nullptr && b.bytes() == 0 && b.error() == Counting::CODE && Counting::live.empty());
    CHECK(b.reserve(5000, 10) == ZSCRC_OK && b.bytes() == 5010 && calls() == 6);
    CHECK(b.error() == Counting::CODE); /* the code of the last failure, also after a success */
    fill(b);
    {
        /* growth that keeps the contents: a larger one is filled, takes the place, and the old one is freed */
        void *old = b.as<void>();
        Scoped next;
        CHECK(next.reserve(2 * 5010) == ZSCRC_OK && calls() == 7 && Counting::live.size() == 2);
        memcpy(next.as<void>(), b.as<void>(), b.bytes());
        void *grown = next.as<void>();
        next.swap(b);
        CHECK(b.as<void>() == grown && b.bytes() == 10020 && next.as<void>() == old && next.bytes() == 5010);
    }
    CHECK(calls() == 8 && !last().alloc && last().bytes == 5010 && Counting::live.size() == 1);
    CHECK(b.as<uint8_t>()[5009] == 0x5A);
    fill(b);
    b.release();
    CHECK(calls() == 9 && !last().alloc && b.bytes() == 0 && b.as<void>() == nullptr);
    b.release(); /* twice: nothing more */
    CHECK(calls() == 9 && Counting::live.empty());
}

static void site_formulas()
{
    static const size_t xs[] = {1, 7, 8, 63, 64, 1000, 4096, 65537, 100003};
    for (const Site &s : sites)
        for (size_t x : xs) {
            Buf b;
            CHECK(b.reserve(s.need(x), s.slack(x)) == ZSCRC_OK && b.bytes() == s.old(x));
            fill(b);
            /* and the group helper with the widths of the host arrays and the descriptors */
            static const size_t width[3] = {8, 8, 4};
            Buf g[3];
            CHECK(zs::reserve_all(g, s.need(x), s.slack(x), width) == ZSCRC_OK);
            for (int i = 0; i < 3; ++i) {
                CHECK(g[i].bytes() == width[i] * s.old(x));
                fill(g[i]);
            }
            const size_t before = calls();
            /* the old conditions: large enough for the need it was grown for, and for what it holds */
            CHECK(zs::reserve_all(g, s.need(x), s.slack(x), width) == ZSCRC_OK && calls() == before);
            CHECK(zs::reserve_all(g, s.old(x), 99, width) == ZSCRC_OK && calls() == before);
            CHECK(zs::reserve_all(g, s.old(x) + 1, 0, width) == ZSCRC_OK && calls() == before + 6);
            for (int i = 0; i < 3; ++i) /* all three freed, then all three allocated */
                CHECK(!Counting::log[before + i].alloc && Counting::log[before + 3 + i].alloc);
            zs::release_all(g);
            b.release();
            CHECK(Counting::live.empty());
        }
}

/* Three buffers of a call; `leave` = the statement after which it returns. */
static int scoped_call(int leave, std::vector<void *> &ptrs)
{
    Scoped a, b;
    if (a.reserve(100) || b.reserve(200))
        return -1;
    ptrs = {a.as<void>(), b.as<void>()};
    fill(a);
    fill(b);
    if (leave == 0)
        return 0; /* the early return */
    Scoped c;
    if (c.reserve(300, 5))
        return -1;
    ptrs.push_back(c.as<void>());
    fill(c);
    if (leave == 1)
        c.release(); /* released by hand: the scope's end frees it no second time */
    return 1;
}

static void scoped_order()
{
    for (int leave = 0; leave < 3; ++leave) {
        std::vector<void *> ptrs;
        const size_t before = calls();
        CHECK(scoped_call(leave, ptrs) == (leave ? 1 : 0));
        const size_t n = ptrs.size();
        CHECK(calls() == before + 2 * n && Counting::live.empty());
        if (leave == 1) { /* c by hand, then b, a */
            CHECK(last(2).p == ptrs[2] && last(1).p == ptrs[1] && last(0).p == ptrs[0]);
        } else { /* the reverse of their declaration */
            for (size_t i = 0; i < n; ++i)
                CHECK(!last(i).alloc && last(i).p == ptrs[i]);
        }
    }
    /* a failure in the middle of a call frees what the call had */
    Counting::fail_in = 2;
    std::vector<void *> ptrs;
    CHECK(scoped_call(2, ptrs) == -1 && Counting::live.empty());
}

static void groups()
{
    constexpr size_t N = 4;
    for (size_t k = 1; k <= N; ++k) {
        Buf g[N];
        CHECK(zs::reserve_all(g, 512) == ZSCRC_OK && Counting::live.size() == N);
        /* growth with the k-th allocation failing: all freed first, those before k kept, the rest empty */
        const size_t before = calls();
        Counting::fail_in = k;
        CHECK(zs::reserve_all(g, 4096, 64) == ZSCRC_ENOMEM);
        CHECK(calls() == before + N + k && Counting::live.size() == k - 1);
        for (size_t i = 0; i < N; ++i) {
            CHECK(!Counting::log[before + i].alloc);
            CHECK(g[i].bytes() == (i < k - 1 ? 4160u : 0u) && (g[i].as<void>() != nullptr) == (i < k - 1));
            fill(g[i]);
        }
        if (k % 2) { /* release after the failure: nothing leaks */
            zs::release_all(g);
            CHECK(Counting::live.empty());
        }
        /* the retry, also for less than what the first ones hold: frees those and allocates all N */
        const size_t retry = calls(), held = Counting::live.size();
        CHECK(zs::reserve_all(g, 1024, 64) == ZSCRC_OK && calls() == retry + held + N);
        for (size_t i = 0; i < N; ++i) {
            CHECK(Counting::log[retry + held + i].alloc && g[i].bytes() == 1088);
            fill(g[i]);
        }
        zs::release_all(g);
        zs::release_all(g);
        CHECK(Counting::live.empty());
    }
}

int main()
{
    reserve_rules();
    site_formulas();
    scoped_order();
    groups();
    CHECK(Counting::live.empty() && Counting::fail_in == 0);
    size_t allocs = 0, frees = 0;
    for (const Call &c : Counting::log)
        (c.alloc ? allocs : frees) += c.p != nullptr;
    CHECK(allocs == frees);
    printf("ok %zu checks, %zu live\n", g_checks, Counting::live.size());
    return 0;
}
