/*
 * Race driver for libzscrc's host side (TEST INFRASTRUCTURE): NTHREADS
 * pthreads start behind a barrier, so that the library's lazily built state
 * (the x^(8*2^k) table of zscrc_gf2.c, the CPU probe, the environment) is
 * first reached by several threads at once, and each loops ROUNDS times over
 * the drop-in CRCs, crc32c_combine / zscrc_shift at many lengths, the
 * zeroskip parsers on the fixture images named in argv and the diagnostics,
 * while thread 0 also flips the process-global tuners the others read.
 *
 * Every thread has the same inputs (private copies), so every round of
 * every thread must give the same digest of all outputs; main computes that
 * digest once more, single-threaded, after the join and exits 1 on any
 * difference.  No device entry point is called and the scalar offload stays
 * off (run with ZSCRC_GPU_MIN=0; the flipped thresholds stay far above any
 * length used here): zscrc_stats' GPU counters must not move.
 *
 * Built plain against libzscrc.so and, under ThreadSanitizer, against the
 * library's host objects (tests/test_thread_race.py).
 *
 * usage: thread_race FILE...   prints {"threads": N, "rounds": R, ...}
 */
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "zscrc.h"

#define NTHREADS 8
#define ROUNDS 300
#define BUF (48u << 10)

static int g_nf;
static unsigned char **g_img; /* the fixtures, read-only after main loaded them */
static size_t *g_sz;
static pthread_barrier_t g_start;

typedef struct {
    int id;
    uint64_t digest; /* of round 0 */
    long differing;  /* rounds whose digest was another */
    int failed;
} worker;

static void mix(uint64_t *h, const void *p, size_t n)
{
    const unsigned char *b = p;
    for (size_t i = 0; i < n; ++i)
        *h = (*h ^ b[i]) * 0x100000001b3ull;
}

static void mix64(uint64_t *h, uint64_t v) { mix(h, &v, sizeof v); }

/* the private inputs of one thread: the same bytes in every thread */
typedef struct {
    unsigned char *buf; /* BUF pseudo-random bytes, none of them 0 */
    unsigned char **img;
    uint64_t *off, *len;
    zscrc_zs_record *rec;
    size_t cap;
} inputs;

static int inputs_init(inputs *in)
{
    in->buf = malloc(BUF + 1);
    in->img = calloc((size_t)g_nf, sizeof *in->img);
    if (!in->buf || !in->img)
        return 0;
    uint64_t s = 0x9e3779b97f4a7c15ull;
    for (size_t i = 0; i < BUF; ++i) {
        s ^= s << 13, s ^= s >> 7, s ^= s << 17;
        in->buf[i] = (unsigned char)(s % 255 + 1);
    }
    in->buf[BUF] = 0;
    in->cap = 0;
    for (int f = 0; f < g_nf; ++f) {
        if (!(in->img[f] = malloc(g_sz[f] ? g_sz[f] : 1)))
            return 0;
        memcpy(in->img[f], g_img[f], g_sz[f]);
        if (g_sz[f] / 8 + 2 > in->cap)
            in->cap = g_sz[f] / 8 + 2;
    }
    in->off = calloc(in->cap, 8);
    in->len = calloc(in->cap, 8);
    in->rec = calloc(in->cap, sizeof *in->rec);
    return in->off && in->len && in->rec;
}

static void inputs_free(inputs *in)
{
    for (int f = 0; in->img && f < g_nf; ++f)
        free(in->img[f]);
    free(in->img);
    free(in->buf);
    free(in->off);
    free(in->len);
    free(in->rec);
}

/* one round: every operation once, all outputs into one digest */
static uint64_t one_round(inputs *in)
{
    uint64_t h = 0xcbf29ce484222325ull;
    /* x^(8n) mod P: every power of two, its neighbours, small and mixed lengths.
     * First in the round: these calls take no lock and touch no atomic, so
     * right behind the barrier nothing orders the threads' first use of the
     * table they build lazily */
    for (int k = 0; k < 64; ++k) {
        const uint64_t n = 1ull << k;
        mix64(&h, zscrc_shift(0x12345678u + (uint32_t)k, n));
        mix64(&h, zscrc_shift(0xdeadbeefu, n - 1));
        mix64(&h, crc32c_combine(0x01020304u * (uint32_t)(k + 1), 0xa5a5a5a5u, n + 1));
        mix64(&h, crc32c_combine(0x0badf00du, (uint32_t)k, n * 0x9e3779b97f4a7c15ull));
    }
    for (uint64_t n = 0; n < 48; ++n)
        mix64(&h, crc32c_combine(0x11111111u, 0x22222222u, n) ^ zscrc_shift(0x33333333u, n));
    crc32c_init();
    /* the drop-in CRCs at a few alignments and lengths, chained */
    static const size_t at[] = {0, 1, 3, 7, 64, 4097}, ln[] = {0, 1, 7, 63, 64, 65, 640, 4096, 30001};
    for (size_t a = 0; a < sizeof at / sizeof *at; ++a)
        for (size_t l = 0; l < sizeof ln / sizeof *ln; ++l) {
            const uint32_t hw = crc32c_hw(0, in->buf + at[a], ln[l]);
            mix64(&h, hw);
            mix64(&h, crc32c_sw(0, in->buf + at[a], ln[l]));
            mix64(&h, crc32c(hw, in->buf + at[a] + ln[l], 100));
        }
    mix64(&h, crc32c_map((const char *)in->buf + 5, 12345));
    mix64(&h, crc32c_buf((const char *)in->buf + (BUF - 2000))); /* NUL at buf[BUF] */
    cstring cs = {3000, 3001, (char *)in->buf + 11};
    mix64(&h, crc32c_cstring(&cs));
    struct iovec iov[3] = {{in->buf, 100}, {in->buf + 100, 0}, {in->buf + 100, 9000}};
    mix64(&h, crc32c_iovec(iov, 3));
    /* the parsers over every fixture */
    for (int f = 0; f < g_nf; ++f) {
        const unsigned char *p = in->img[f];
        const uint64_t n = g_sz[f];
        size_t nc = 0;
        uint64_t end = 0;
        const int wr = zscrc_zs_walk(p, n, in->off, in->len, in->cap, &nc, &end);
        mix64(&h, (uint64_t)wr);
        if (wr >= 0) {
            const size_t got = nc < in->cap ? nc : in->cap;
            mix64(&h, nc);
            mix64(&h, end);
            mix(&h, in->off, 8 * got);
            mix(&h, in->len, 8 * got);
        }
        uint64_t po[2] = {0, 0}, pl[2] = {0, 0};
        const int pr = zscrc_zs_packed_spans(p, n, po, pl);
        mix64(&h, (uint64_t)pr);
        if (pr == ZSCRC_OK) {
            mix(&h, po, sizeof po);
            mix(&h, pl, sizeof pl);
        }
        for (int kind = 0; kind < 3; ++kind) {
            size_t nr = 0;
            const int rr = zscrc_zs_records(p, n, kind, in->rec, in->cap, &nr);
            mix64(&h, (uint64_t)rr);
            if (rr >= 0) {
                mix64(&h, nr);
                mix(&h, in->rec, sizeof *in->rec * (nr < in->cap ? nr : in->cap));
            }
        }
        uint32_t st = 0, cp = 0;
        int rc = zscrc_zs_header_crc(p, n, &st, &cp);
        mix64(&h, (uint64_t)rc);
        if (rc >= 0)
            mix64(&h, ((uint64_t)st << 32) | cp);
        st = cp = 0;
        rc = zscrc_zs_dotzsdb_crc(p, n, &st, &cp);
        mix64(&h, (uint64_t)rc);
        if (rc >= 0)
            mix64(&h, ((uint64_t)st << 32) | cp);
    }
    uint8_t db[61];
    memset(db, 0, sizeof db);
    mix64(&h, (uint64_t)zscrc_zs_dotzsdb_build(4096, "00010203-0405-0607-0809-0a0b0c0d0e0f", 8, db));
    mix(&h, db, sizeof db);
    /* diagnostics: the values move with the other threads' calls, so only
     * called, and the GPU's counters checked to stay put */
    uint64_t stats[4];
    zscrc_stats(stats);
    if (!zscrc_last_error() || stats[1] || stats[2] || stats[3])
        h = 0;
    return h;
}

static void flip_tuners(int round)
{
    /* thresholds far above every length used here: no call offloads */
    if (round & 1)
        zscrc_set_gpu_min_pair(1ull << 40, 1ull << 41);
    else
        zscrc_set_gpu_min_pair(0, 0);
    zscrc_set_teams(round % 3 ? 640 : 256, round % 5 ? 1u << 20 : 64u << 10);
    zscrc_set_opt((unsigned)round & 3u);
}

static void *run(void *arg)
{
    worker *w = arg;
    inputs in;
    memset(&in, 0, sizeof in);
    w->failed = !inputs_init(&in);
    pthread_barrier_wait(&g_start);
    for (int r = 0; !w->failed && r < ROUNDS; ++r) {
        if (w->id == 0)
            flip_tuners(r);
        const uint64_t d = one_round(&in);
        if (r == 0)
            w->digest = d;
        else if (d != w->digest)
            ++w->differing;
    }
    inputs_free(&in);
    return NULL;
}

static unsigned char *load(const char *path, size_t *n)
{
    FILE *fp = fopen(path, "rb");
    if (!fp)
        return NULL;
    fseek(fp, 0, SEEK_END);
    *n = (size_t)ftell(fp);
    fseek(fp, 0, SEEK_SET);
    unsigned char *p = malloc(*n ? *n : 1);
    if (p && fread(p, 1, *n, fp) != *n) {
        free(p);
        p = NULL;
    }
    fclose(fp);
    return p;
}

int main(int argc, char **argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: %s FILE...\n", argv[0]);
        return 2;
    }
    g_nf = argc - 1;
    g_img = calloc((size_t)g_nf, sizeof *g_img);
    g_sz = calloc((size_t)g_nf, sizeof *g_sz);
    for (int f = 0; f < g_nf; ++f)
        if (!(g_img[f] = load(argv[1 + f], &g_sz[f]))) {
            perror(argv[1 + f]);
            return 2;
        }
    /* no library call before the threads: the first calls are theirs */
    pthread_t th[NTHREADS];
    worker w[NTHREADS];
    memset(w, 0, sizeof w);
    pthread_barrier_init(&g_start, NULL, NTHREADS);
    for (int t = 0; t < NTHREADS; ++t) {
        w[t].id = t;
        if (pthread_create(&th[t], NULL, run, &w[t])) {
            perror("pthread_create");
            return 2;
        }
    }
    for (int t = 0; t < NTHREADS; ++t)
        pthread_join(th[t], NULL);
    pthread_barrier_destroy(&g_start);
    /* the tuners back at their defaults (the thresholds: ZSCRC_GPU_MIN=0) */
    const char *e = getenv("ZSCRC_GPU_MIN");
    const uint64_t gmin = e ? strtoull(e, NULL, 0) : 0;
    zscrc_set_gpu_min_pair(gmin, gmin);
    zscrc_set_teams(640, 1u << 20);
    zscrc_set_opt(0);
    /* the same round once more, alone */
    inputs in;
    memset(&in, 0, sizeof in);
    if (!inputs_init(&in))
        return 2;
    const uint64_t want = one_round(&in);
    inputs_free(&in);
    int bad = want == 0;
    for (int t = 0; t < NTHREADS; ++t)
        if (w[t].failed || w[t].differing || w[t].digest != want) {
            ++bad;
            fprintf(stderr, "thread %d: digest %016llx, single-threaded %016llx, %ld differing rounds%s\n", t,
                    (unsigned long long)w[t].digest, (unsigned long long)want, w[t].differing,
                    w[t].failed ? ", setup failed" : "");
        }
    printf("{\"threads\": %d, \"rounds\": %d, \"digest\": \"%016llx\", \"mismatches\": %d}\n", NTHREADS, ROUNDS,
           (unsigned long long)want, bad);
    for (int f = 0; f < g_nf; ++f)
        free(g_img[f]);
    free(g_img);
    free(g_sz);
    return bad ? 1 : 0;
}
