// buf_host.cpp -- wl::Buf (waterlily_amd/csrc/wl_buf.h) on the host, over malloc, under the address and undefined-behaviour
// sanitizers (tests/test_buf_cpu.py compiles and runs this).  The policy counts live blocks and fails the k-th allocation on
// request: the only place the library's partial-failure paths can be exercised.  Exit status 0: every check held.
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "wl_buf.h"

struct TestMem {
    static int live, allocs, frees, fail_at;   // fail_at: the allocation (counted from 1, from the last arm()) that fails; 0: none
    static size_t last_bytes;
    static void arm(int k) { allocs = 0; frees = 0; fail_at = k; }
    static int alloc(void **p, size_t bytes) {
        allocs += 1;
        if (allocs == fail_at) return 2;   // (hipErrorOutOfMemory's number; any non-zero code)
        *p = malloc(bytes);
        if (!*p) return 2;
        live += 1;
        last_bytes = bytes;
        return 0;
    }
    static void free(void *p) { ::free(p); live -= 1; frees += 1; }
};
int TestMem::live = 0, TestMem::allocs = 0, TestMem::frees = 0, TestMem::fail_at = 0;
size_t TestMem::last_bytes = 0;

template <class T> using B = wl::Buf<T, TestMem>;

static int failed = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { fprintf(stderr, "buf_host.cpp:%d: %s\n", __LINE__, #cond); failed += 1; } \
    } while (0)

// the shape of measure_alloc: five arrays of one flow handle, reserved in order, the first error returned
struct Five {
    B<int> rowcount;
    B<long> rowoff;
    B<unsigned char> touched, prev, changed;
    int alloc(size_t nrows) {
        if (int rc = rowcount.reserve(nrows)) return rc;
        if (int rc = rowoff.reserve(nrows + 1)) return rc;
        if (int rc = touched.reserve(nrows)) return rc;
        if (int rc = prev.reserve(nrows)) return rc;
        return changed.reserve(nrows);
    }
};

int main() {
    // (a) reserve, then destruction
    TestMem::arm(0);
    {
        B<double> b;
        CHECK(b.get() == nullptr && b.count() == 0);
        CHECK(b.reserve(100) == 0);
        CHECK(b.get() != nullptr && b.count() == 100 && TestMem::live == 1 && TestMem::last_bytes == 100 * sizeof(double));
        b.get()[99] = 1.0;   // (the sanitizer checks the block is that large)
    }
    CHECK(TestMem::live == 0 && TestMem::allocs == 1 && TestMem::frees == 1);

    // (b) a reserve that fits allocates nothing and keeps the pointer
    TestMem::arm(0);
    {
        B<int> b;
        CHECK(b.reserve(64) == 0);
        int *p = b.get();
        CHECK(b.reserve(64) == 0 && b.reserve(1) == 0 && b.reserve(0) == 0 && b.reserve(10, 1000) == 0);
        CHECK(b.get() == p && b.count() == 64 && TestMem::allocs == 1 && TestMem::frees == 0);
    }
    CHECK(TestMem::live == 0);
    {
        B<int> b;   // nothing asked for, nothing allocated
        CHECK(b.reserve(0) == 0 && b.reserve(0, 64) == 0 && b.get() == nullptr && TestMem::live == 0);
    }

    // (c) growth frees the old block exactly once and reports the new count; grow_to with the busy list's numbers
    TestMem::arm(0);
    {
        B<int> b;
        CHECK(b.reserve(8) == 0);
        CHECK(b.reserve(9) == 0);
        CHECK(b.count() == 9 && TestMem::allocs == 2 && TestMem::frees == 1 && TestMem::live == 1);
        b.get()[8] = 7;
        b.reset();
        CHECK(b.get() == nullptr && b.count() == 0 && TestMem::live == 0 && TestMem::frees == 2);
        b.reset();   // (idempotent)
        CHECK(TestMem::frees == 2);
    }
    TestMem::arm(0);
    {
        B<int> busy;
        CHECK(busy.reserve(1, 64) == 0 && busy.count() == 64);                  // no busy row: 64 entries
        CHECK(busy.reserve(1, 64) == 0 && busy.reserve(64, 2 * 64 + 64) == 0);  // fits: untouched
        CHECK(busy.count() == 64 && TestMem::allocs == 1);
        CHECK(busy.reserve(100, 2 * 100 + 64) == 0);                            // 100 rows do not fit: 2 n + 64
        CHECK(busy.count() == 264 && TestMem::last_bytes == 264 * sizeof(int) && TestMem::allocs == 2 && TestMem::frees == 1);
        busy.get()[263] = 1;
        CHECK(busy.reserve(264, 2 * 264 + 64) == 0 && TestMem::allocs == 2);
        CHECK(busy.reserve(5, 2) == 0 && busy.count() == 264);
    }
    CHECK(TestMem::live == 0);
    {
        B<char> pin;   // grow_to below count: count wins
        CHECK(pin.reserve(10, 4) == 0 && pin.count() == 10);
    }

    // (d) a growing reserve whose allocation fails
    TestMem::arm(0);
    {
        B<long> b;
        CHECK(b.reserve(16) == 0);
        TestMem::arm(1);
        CHECK(b.reserve(32) != 0);
        CHECK(b.get() == nullptr && b.count() == 0 && TestMem::live == 0 && TestMem::frees == 1);
        // (the allocator is healthy again: only allocation 1 since arm(1) fails)
        CHECK(b.reserve(32) == 0 && b.get() != nullptr && b.count() == 32 && TestMem::live == 1);
        b.get()[31] = 1;
    }
    CHECK(TestMem::live == 0);
    TestMem::arm(1);
    {
        B<long> b;   // the first allocation of an empty buffer fails
        CHECK(b.reserve(4, 64) == 2 && b.get() == nullptr && b.count() == 0 && TestMem::live == 0 && TestMem::frees == 0);
        CHECK(b.reserve(4, 64) == 0 && b.count() == 64 && TestMem::live == 1);
    }
    CHECK(TestMem::live == 0);

    // (e) moves empty the source and free the target's old block once
    TestMem::arm(0);
    {
        B<int> a;
        CHECK(a.reserve(10) == 0);
        int *pa = a.get();
        B<int> b(std::move(a));
        CHECK(a.get() == nullptr && a.count() == 0 && b.get() == pa && b.count() == 10 && TestMem::live == 1 && TestMem::frees == 0);
        B<int> c;
        CHECK(c.reserve(20) == 0 && TestMem::live == 2);
        c = std::move(b);
        CHECK(b.get() == nullptr && b.count() == 0 && c.get() == pa && c.count() == 10 && TestMem::live == 1 && TestMem::frees == 1);
        B<int> &self = c;
        c = std::move(self);
        CHECK(c.get() == pa && c.count() == 10 && TestMem::live == 1 && TestMem::frees == 1);
        B<int> e;
        c = std::move(e);   // an empty source frees the target
        CHECK(c.get() == nullptr && c.count() == 0 && TestMem::live == 0 && TestMem::frees == 2);
    }
    CHECK(TestMem::live == 0 && TestMem::frees == 2);

    // (f) five buffers, the third allocation fails; the retry completes the set
    const size_t nrows = 37;
    {
        Five f;
        TestMem::arm(3);
        CHECK(f.alloc(nrows) != 0);
        CHECK(TestMem::live == 2 && f.rowcount.count() == nrows && f.rowoff.count() == nrows + 1);
        CHECK(f.touched.get() == nullptr && f.touched.count() == 0 && f.prev.get() == nullptr && f.changed.get() == nullptr);
        int *kept = f.rowcount.get();
        TestMem::arm(0);
        CHECK(f.alloc(nrows) == 0);
        CHECK(TestMem::allocs == 3 && TestMem::frees == 0 && TestMem::live == 5 && f.rowcount.get() == kept);
        CHECK(f.rowcount.count() == nrows && f.rowoff.count() == nrows + 1 && f.touched.count() == nrows && f.prev.count() == nrows &&
              f.changed.count() == nrows);
        CHECK(f.rowcount.get() && f.rowoff.get() && f.touched.get() && f.prev.get() && f.changed.get());
        f.rowoff.get()[nrows] = 0;
        f.changed.get()[nrows - 1] = 0;
        CHECK(f.alloc(nrows) == 0 && TestMem::allocs == 3);
    }
    CHECK(TestMem::live == 0);

    if (failed) { fprintf(stderr, "buf_host: %d check(s) failed\n", failed); return 1; }
    printf("buf_host ok\n");
    return 0;
}
