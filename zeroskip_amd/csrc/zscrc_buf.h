/*
 * zscrc_buf.h -- zs::Buf, the one owner of device and pinned host memory in
 * the host library: a pointer and its byte count that grow by the rule every
 * cached buffer follows (nothing to do when large enough; else free first, so
 * the peak does not rise, then allocate with the site's slack; empty after a
 * failure) and that are freed in one place.  Mem is the backend: two static
 * functions, alloc(void **, size_t) returning 0 or the backend's error code,
 * and free(void *).  The two HIP backends are in zscrc_buf_hip.h.  Host code,
 * plain C++: tests/c/devbuf.cpp includes this header alone, with a counting
 * malloc backend.
 */
#ifndef ZSCRC_BUF_H
#define ZSCRC_BUF_H

#include <stddef.h>

#include <type_traits>
#include <utility>

#include "../../include/zscrc.h"

namespace zs {

/* A cached buffer: a member of an object of static storage (or of a handle),
 * released by that object's release function and never by a destructor -- no
 * backend call runs from a static destructor at process exit. */
template <class Mem>
class Buf {
public:
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;

    /* At least `need` bytes; contents are dropped when it grows, to
     * need + slack bytes.  ZSCRC_OK or, the buffer then empty, ZSCRC_ENOMEM
     * (the backend's code: error()). */
    int reserve(size_t need, size_t slack = 0)
    {
        if (bytes_ >= need)
            return ZSCRC_OK;
        release();
        if (const int e = Mem::alloc(&p_, need + slack)) {
            err_ = e;
            p_ = nullptr;
            return ZSCRC_ENOMEM;
        }
        bytes_ = need + slack;
        return ZSCRC_OK;
    }

    void release()
    {
        static_assert(std::is_trivially_destructible<Buf>::value, "a cached Buf frees nothing at process exit");
        if (p_)
            Mem::free(p_);
        p_ = nullptr;
        bytes_ = 0;
    }

    /* The two exchange what they own: a grown copy takes the old one's place. */
    void swap(Buf &o)
    {
        std::swap(p_, o.p_);
        std::swap(bytes_, o.bytes_);
    }

    template <class T>
    T *as() const
    {
        return static_cast<T *>(p_);
    }
    size_t bytes() const { return bytes_; }
    /* the backend's code of the last reserve() that failed */
    int error() const { return err_; }

private:
    void *p_ = nullptr;
    size_t bytes_ = 0;
    int err_ = 0;
};

/* A call's own buffer: released at the end of its scope. */
template <class Mem>
class ScopedBuf : public Buf<Mem> {
public:
    ScopedBuf() = default;
    ~ScopedBuf() { this->release(); }
};

template <class Mem, size_t N>
void release_all(Buf<Mem> (&b)[N])
{
    for (Buf<Mem> &x : b)
        x.release();
}

/* A group of buffers that grow together, b[i] to hold need x width[i] bytes
 * (width NULL: `need` bytes each): nothing to do when every one does; else all
 * are freed, then allocated with slack x width[i] more.  A failure part-way
 * keeps what was allocated before it and leaves the rest empty, so the next
 * call frees and allocates all again. */
template <class Mem, size_t N>
int reserve_all(Buf<Mem> (&b)[N], size_t need, size_t slack = 0, const size_t *width = nullptr)
{
    const auto w = [width](size_t i) { return width ? width[i] : 1; };
    size_t large = 0;
    for (size_t i = 0; i < N; ++i)
        large += b[i].bytes() >= need * w(i);
    if (large == N)
        return ZSCRC_OK;
    release_all(b);
    for (size_t i = 0; i < N; ++i)
        if (const int rc = b[i].reserve(need * w(i), slack * w(i)))
            return rc;
    return ZSCRC_OK;
}

} /* namespace zs */

#endif
