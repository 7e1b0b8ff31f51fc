// wl_buf.h -- Buf<T, Mem>: the one owner of memory the library allocates (device or pinned host).
//
// A Buf is either empty (nullptr, 0) or holds a block of count() elements; pointer and count never disagree, whatever
// an allocation does.  Mem is a policy: static int alloc(void **, size_t bytes) returning 0 or an error code, and
// static void free(void *).  wl_common.h has the real ones (DevMem, PinnedMem); nothing here needs HIP, so a host
// compiler can build and test the type alone (tests/buf_host.cpp).
#pragma once
#include <cstddef>

namespace wl {

template <class T, class Mem> struct Buf {
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    Buf(Buf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    Buf &operator=(Buf &&o) noexcept {
        if (this != &o) { reset(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
        return *this;
    }
    ~Buf() { reset(); }
    // room for `count` elements; a block that has to grow is allocated with max(count, grow_to).  The old CONTENT IS LOST.
    // On failure: the allocator's error code, and the buffer is empty.
    int reserve(size_t count, size_t grow_to = 0) {
        if (count <= n) return 0;
        reset();
        const size_t want = count > grow_to ? count : grow_to;
        void *q = nullptr;
        const int rc = Mem::alloc(&q, want * sizeof(T));
        if (rc) return rc;
        p = (T *)q; n = want;
        return 0;
    }
    void reset() {
        if (p) Mem::free(p);
        p = nullptr; n = 0;
    }
    T *get() const { return p; }
    size_t count() const { return n; }

  private:
    T *p = nullptr;
    size_t n = 0;
};

}  // namespace wl
