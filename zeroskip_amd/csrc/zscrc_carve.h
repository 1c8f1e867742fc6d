/*
 * zscrc_carve.h -- zs::Carve, the scratch layout of a device stage's call
 * (part of zscrc_internal.h).  A stage has one function that takes its pieces
 * out of a Carve in order: on a NULL base it sizes the scratch, on the buffer
 * it sets the kernels' pointers, so the two cannot differ.  Host code, plain
 * C++: tests/c/carve.cpp includes it alone.
 */
#ifndef ZSCRC_CARVE_H
#define ZSCRC_CARVE_H

#include <stddef.h>
#include <stdint.h>

namespace zs {

class Carve {
public:
    /* base: aligned to the largest alignment asked of take(), or NULL */
    explicit Carve(void *base) : base_(reinterpret_cast<uintptr_t>(base)) {}

    /* The next piece: count x T at a multiple of align (a power of two); NULL on a NULL base. */
    template <class T>
    T *take(size_t count, size_t align = alignof(T))
    {
        at_ = (at_ + align - 1) & ~(align - 1);
        T *p = base_ ? reinterpret_cast<T *>(base_ + at_) : nullptr;
        at_ += count * sizeof(T);
        return p;
    }

    /* up to the end of the last piece */
    size_t bytes() const { return at_; }

private:
    uintptr_t base_;
    size_t at_ = 0;
};

} /* namespace zs */

#endif
