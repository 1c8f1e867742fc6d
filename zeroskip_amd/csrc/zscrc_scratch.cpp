/*
 * zscrc_scratch.cpp -- the library-owned scratch of the device stages
 * (zs::Scratch, zscrc_internal.h): one buffer and one pinned staging per
 * device, shared by every call there that passes no scratch of its own
 * (zscrc_device_walk, _records, _walk_multi, _pack, _merge).  A call on another
 * stream than the last user's waits for that user's work.  The calls reach it
 * through zs::with_scratch (zscrc_internal.h).  Also the host code the stages
 * share that calls HIP: the check and the staging of a call's record lists
 * (zscrc_lists.h) and the grid of the tiled copies (zsdev::copy_grid).
 */
#include <hip/hip_runtime.h>

#include <mutex>

#include "../../include/zscrc.h"
#include "zscrc_internal.h"
#include "zscrc_lists.h"

namespace {

constexpr int MAX_DEV = 64;
zs::Scratch g_scratch[MAX_DEV];

} /* namespace */

namespace zs {

Scratch *device_scratch()
{
    int dev = -1;
    return hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < MAX_DEV ? &g_scratch[dev] : nullptr;
}

int scratch_acquire(Scratch &sc, size_t need, hipStream_t s)
{
    if (sc.buf.bytes() < need) {
        sc.last_valid = false;
        /* the free waits for the device: no user is left; about the image's size: no slack on top */
        if (const int rc = sc.buf.reserve(need))
            return rc;
    }
    /* a wait on the stream's own event is harmless: "not certainly the same stream" waits */
    if (sc.last_valid && !zs::same_stream(sc.last_stream, s) && hipStreamWaitEvent(s, sc.last, 0) != hipSuccess)
        return ZSCRC_EHIP;
    return ZSCRC_OK;
}

int scratch_done(Scratch &sc, hipStream_t s, int rc)
{
    if (!sc.last && hipEventCreateWithFlags(&sc.last, hipEventDisableTiming) != hipSuccess)
        sc.last = nullptr;
    sc.last_valid = sc.last && hipEventRecord(sc.last, s) == hipSuccess;
    sc.last_stream = s;
    if (!sc.last_valid && rc == ZSCRC_OK) /* no event to order the next user by: drain instead */
        return hipStreamSynchronize(s) == hipSuccess ? ZSCRC_OK : ZSCRC_EHIP;
    return rc;
}

int stage_begin(Scratch &sc, size_t bytes)
{
    /* the staging's last copy must have run before its bytes change */
    if (sc.staged_valid && hipEventSynchronize(sc.staged) != hipSuccess)
        return ZSCRC_EHIP;
    sc.staged_valid = false;
    return sc.pin.reserve(bytes);
}

int stage_copy(Scratch &sc, void *d_dst, size_t bytes, hipStream_t s)
{
    if (hipMemcpyAsync(d_dst, sc.pin.as<void>(), bytes, hipMemcpyHostToDevice, s) != hipSuccess)
        return ZSCRC_EHIP;
    if (!sc.staged && hipEventCreateWithFlags(&sc.staged, hipEventDisableTiming) != hipSuccess)
        sc.staged = nullptr;
    sc.staged_valid = sc.staged && hipEventRecord(sc.staged, s) == hipSuccess;
    if (!sc.staged_valid) /* no event to wait for before the next fill: drain instead */
        return hipStreamSynchronize(s) == hipSuccess ? ZSCRC_OK : ZSCRC_EHIP;
    return ZSCRC_OK;
}

} /* namespace zs */

/* zscrc_lists.h, and the grid of the tiled copies (zscrc_internal.h) */
namespace zsdev {

bool lists_ok(const zscrc_merge_list *lists, size_t k, size_t kmax, uint64_t *n_total, uint32_t *filled)
{
    if ((k && !lists) || k > kmax)
        return false;
    uint64_t n = 0;
    *filled = 0;
    for (size_t l = 0; l < k; ++l) {
        if ((lists[l].n && !lists[l].d_recs) || lists[l].n > N_MAX - n)
            return false;
        n += lists[l].n;
        *filled += lists[l].n != 0;
    }
    *n_total = n;
    return true;
}

int stage_lists(zs::Scratch &sc, const zscrc_merge_list *lists, size_t k, uint32_t filled, ListD *d_dst,
                hipStream_t s)
{
    const size_t bytes = ((size_t)filled + 1) * sizeof(ListD);
    const int rc = zs::stage_begin(sc, bytes);
    if (rc)
        return rc;
    ListD *h = sc.pin.as<ListD>();
    uint64_t first = 0;
    for (size_t l = 0; l < k; ++l) {
        if (!lists[l].n)
            continue;
        *h++ = ListD{lists[l].d_recs, first, lists[l].base};
        first += lists[l].n;
    }
    *h = ListD{nullptr, first, 0};
    return zs::stage_copy(sc, d_dst, bytes, s);
}

int copy_grid(uint64_t out_cap, uint64_t tile, unsigned wg_per_cu, unsigned *grid)
{
    int dev = 0, ncu = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu <= 0)
        return ZSCRC_EHIP;
    const uint64_t g = (out_cap + tile - 1) / tile, gmax = (uint64_t)ncu * wg_per_cu;
    *grid = (unsigned)(g < gmax ? g : gmax);
    return ZSCRC_OK;
}

} /* namespace zsdev */

/* zscrc_release_cache(): the scratch and the staging, every device. */
extern "C" void zs_walk_release_cache(void)
{
    int cur = -1;
    (void)hipGetDevice(&cur);
    for (int d = 0; d < MAX_DEV; ++d) {
        zs::Scratch &sc = g_scratch[d];
        std::lock_guard<std::mutex> lk(sc.mu);
        if (!sc.buf.bytes() && !sc.last && !sc.pin.bytes() && !sc.staged)
            continue;
        (void)hipSetDevice(d);
        sc.buf.release();
        if (sc.last)
            (void)hipEventDestroy(sc.last);
        if (sc.staged_valid)
            (void)hipEventSynchronize(sc.staged);
        sc.pin.release();
        if (sc.staged)
            (void)hipEventDestroy(sc.staged);
        sc.last = nullptr;
        sc.last_valid = false;
        sc.staged = nullptr;
        sc.staged_valid = false;
    }
    if (cur >= 0)
        (void)hipSetDevice(cur);
}
