// lk_internal.h -- symbols shared between the translation units of liblightkrylov_hip.so (not part of the ABI).
#pragma once
#include "../../include/lightkrylov_hip.h"
#include <hip/hip_runtime.h>
#include <utility>

// records the message returned by lk_last_error() and returns `code`
extern "C" int lk_fail_(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3), visibility("hidden")));

namespace lk {

// Owner of one allocation of `T`s: device memory (PINNED = false, hipMalloc / hipFree) or pinned host memory (PINNED = true,
// hipHostMalloc / hipHostFree).  Move-only; reads as a plain `T *` wherever one is expected.  Every allocation and every release of the
// engine goes through this type.
//   reserve(n): at least n elements.  Large enough already: one integer compare.  Otherwise the old block is released FIRST, with the
//   synchronising free (kernels still reading it are safe only because hipFree waits), and exactly n elements are allocated: the contents
//   do not survive growth.  After a failed allocation the owner is empty, capacity 0 -- the next reserve tries again.
//   wrap(p): a non-owning view of caller memory, never freed (capacity 0: it cannot be reserved on).
template <class T, bool PINNED>
class Buf {
    T *p_ = nullptr;
    int64_t cap_ = 0;   // elements
    bool own_ = true;

public:
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    Buf(Buf &&o) noexcept : p_(o.p_), cap_(o.cap_), own_(o.own_) { o.p_ = nullptr; o.cap_ = 0; o.own_ = true; }
    Buf &operator=(Buf &&o) noexcept {
        if (this != &o) { release(); std::swap(p_, o.p_); std::swap(cap_, o.cap_); std::swap(own_, o.own_); }
        return *this;
    }
    ~Buf() { release(); }

    operator T *() const { return p_; }
    T *get() const { return p_; }   // where a template deduces its argument type
    int64_t capacity() const { return cap_; }
    bool owns() const { return own_; }
    void wrap(T *p) { release(); p_ = p; own_ = false; }
    void release() {
        if (p_ && own_) (void)(PINNED ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr; cap_ = 0; own_ = true;
    }
    int reserve(int64_t n) { return n <= cap_ ? LK_OK : grow(n); }

private:
    int grow(int64_t n) {
        release();
        const size_t bytes = (size_t)n * sizeof(T);
        const hipError_t e = PINNED ? hipHostMalloc((void **)&p_, bytes, hipHostMallocDefault) : hipMalloc((void **)&p_, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();   // the runtime's last-error state is sticky: the next launch check must not report this
            p_ = nullptr;
            return lk_fail_(e == hipErrorOutOfMemory ? LK_ERR_NOMEM : LK_ERR_HIP, "%s(%zu bytes) failed: %s", PINNED ? "hipHostMalloc" : "hipMalloc", bytes,
                            hipGetErrorString(e));
        }
        cap_ = n;
        return LK_OK;
    }
};
template <class T> using DevBuf = Buf<T, false>;
template <class T> using PinnedBuf = Buf<T, true>;

}  // namespace lk
