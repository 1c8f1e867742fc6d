/* zscrc_buf_hip.h -- the two HIP backends of zs::Buf (zscrc_buf.h): device
 * memory and pinned host memory.  The only hipMalloc / hipHostMalloc /
 * hipFree / hipHostFree calls of the library. */
#ifndef ZSCRC_BUF_HIP_H
#define ZSCRC_BUF_HIP_H

#include <hip/hip_runtime_api.h>

#include "zscrc_buf.h"

namespace zs {

struct Device {
    static int alloc(void **p, size_t n) { return (int)hipMalloc(p, n); }
    static void free(void *p) { (void)hipFree(p); }
};
struct Pinned {
    static int alloc(void **p, size_t n) { return (int)hipHostMalloc(p, n, hipHostMallocDefault); }
    static void free(void *p) { (void)hipHostFree(p); }
};
using DevBuf = Buf<Device>;
using PinBuf = Buf<Pinned>;

/* reserve() for a chain of HIP calls that carries a hipError_t */
template <class Mem>
hipError_t reserve_hip(Buf<Mem> &b, size_t need)
{
    return b.reserve(need) ? (hipError_t)b.error() : hipSuccess;
}

} /* namespace zs */

#endif
