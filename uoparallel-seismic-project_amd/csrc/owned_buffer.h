// owned_buffer.h - an owner of one block of memory that a runtime hands out.  Today it owns the block of a call's
// Scratch (DevBuf of ttsweep_ctx.h); the context's own pools are still raw pointers.  Nothing of HIP here: the memory
// comes from a policy, so that a stand-alone program can check the class on the CPU over malloc / free
// (tests/host/owned_buffer_main.cpp, under the sanitizers).
#pragma once

#include <cstddef>

namespace ttsweep {

// Mem: static int alloc(void **p, size_t bytes) and static int release(void *p), 0 on success, else the runtime's
// error code, which is handed on unchanged.  After a failed alloc(), reserve() or reset() the buffer is empty: the
// pointer is dropped before the release is judged, so no pointer reaches Mem::release twice.  Growing keeps no contents.
template <class T, class Mem>
class OwnedBuffer {
    T *p = nullptr;
    size_t n = 0;

public:
    OwnedBuffer() = default;
    OwnedBuffer(OwnedBuffer &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    OwnedBuffer &operator=(OwnedBuffer &&o) noexcept
    {
        if (this != &o) {
            (void)reset();
            p = o.p; n = o.n;
            o.p = nullptr; o.n = 0;
        }
        return *this;
    }
    ~OwnedBuffer() { (void)reset(); }

    T *get() const { return p; }
    operator T *() const { return p; }
    size_t count() const { return n; }      // elements allocated

    int reset()
    {
        T *const old = p;
        p = nullptr;
        n = 0;
        return old ? Mem::release(old) : 0;
    }
    int alloc(size_t count)                 // exactly `count` elements, whatever was held before
    {
        if (const int e = reset()) return e;
        if (count == 0) return 0;
        void *q = nullptr;
        if (const int e = Mem::alloc(&q, count * sizeof(T))) return e;
        p = static_cast<T *>(q);
        n = count;
        return 0;
    }
    int reserve(size_t count) { return count <= n ? 0 : alloc(count); }
};

} // namespace ttsweep
