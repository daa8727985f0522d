// Buf<T, Mem> (orb-slam-birdview_amd/csrc/buf.h) over a counting malloc policy: what every owner of device and pinned
// memory in the library relies on.  A stand-alone program, built with -fsanitize=address,undefined by
// tests/test_buf_host.py: a double free or a use of a freed block ends it with a report, a failed check (the policy's
// live count among them: a leak) with "violation" and exit status 1; "ok" is the last line otherwise.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <utility>

#include "../../orb-slam-birdview_amd/csrc/buf.h"

namespace {

struct CountingMem {
    static inline int allocs = 0, frees = 0, live = 0, fail_next = 0;
    static inline size_t last_bytes = 0;
    static int alloc(void** p, size_t bytes) {
        if (fail_next) {
            fail_next = 0;
            *p = nullptr;
            return 2;   // (hipErrorOutOfMemory's value; any non-zero is a failure)
        }
        *p = std::malloc(bytes ? bytes : 1);
        if (!*p) return 2;
        std::memset(*p, 0xA5, bytes);
        allocs++;
        live++;
        last_bytes = bytes;
        return 0;
    }
    static void free(void* p) {
        std::free(p);
        frees++;
        live--;
    }
};
using M = CountingMem;
template <class T>
using TBuf = orbgpu::Buf<T, CountingMem>;

static_assert(!std::is_copy_constructible<TBuf<int>>::value && !std::is_copy_assignable<TBuf<int>>::value,
              "Buf is move-only");
static_assert(!std::is_convertible<TBuf<int>, int*>::value && !std::is_convertible<TBuf<int>, bool>::value,
              "no implicit conversion to the pointer (or to bool)");
static_assert(std::is_nothrow_move_constructible<TBuf<int>>::value, "moves do not throw");

int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("violation %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                      \
        }                                                                    \
    } while (0)

// allocations and frees since the last call
struct Delta {
    int a = M::allocs, f = M::frees;
    bool is(int da, int df) {
        const bool ok = M::allocs - a == da && M::frees - f == df;
        a = M::allocs;
        f = M::frees;
        return ok;
    }
};

void reuse_and_growth() {
    TBuf<uint32_t> b;
    CHECK(!b && b.get() == nullptr && b.cap() == 0);
    Delta d;
    // the first allocation honours the floor
    CHECK(b.ensure(10, 256) == 0 && b && b.cap() == 256 && M::last_bytes == 256 * sizeof(uint32_t) && d.is(1, 0));
    uint32_t* const p = b.get();
    p[255] = 7;   // (the whole block is the buffer's: the sanitizer watches the write)
    // 1. n <= cap(): the pointer stays, nothing is allocated or freed; a smaller or larger floor changes nothing
    CHECK(b.ensure(1) == 0 && b.ensure(256) == 0 && b.ensure(200, 4096) == 0 && b.ensure(0) == 0);
    CHECK(b.get() == p && b.cap() == 256 && p[255] == 7 && d.is(0, 0));
    // 2. a larger n: exactly one free and one allocation, of max(n, floor) elements
    CHECK(b.ensure(257, 256) == 0 && b.cap() == 257 && M::last_bytes == 257 * sizeof(uint32_t) && d.is(1, 1));
    CHECK(b.ensure(300, 1000) == 0 && b.cap() == 1000 && M::last_bytes == 1000 * sizeof(uint32_t) && d.is(1, 1));
    b.get()[999] = 1;
    // exact (no floor), and an empty buffer allocates even for n below the old capacity
    CHECK(b.ensure(1001) == 0 && b.cap() == 1001 && d.is(1, 1));
    b.reset();
    CHECK(!b && b.cap() == 0 && d.is(0, 1) && M::live == 0);
    CHECK(b.ensure(5) == 0 && b.cap() == 5 && d.is(1, 0));
}   // 6. the destructor frees (checked by the caller through the live count)

void failed_allocation() {
    TBuf<double> b;
    Delta d;
    // 3. a failure on an empty buffer
    M::fail_next = 1;
    CHECK(b.ensure(8) != 0 && !b && b.get() == nullptr && b.cap() == 0 && d.is(0, 0));
    CHECK(b.ensure(8) == 0 && b && b.cap() == 8 && d.is(1, 0));
    // a failure while growing: the old block is gone (freed once), the buffer empty, and a later ensure succeeds
    M::fail_next = 1;
    CHECK(b.ensure(9, 64) != 0 && !b && b.get() == nullptr && b.cap() == 0 && d.is(0, 1) && M::live == 0);
    CHECK(b.ensure(2, 64) == 0 && b && b.cap() == 64 && d.is(1, 0));
    b.get()[63] = 1.0;
    // a request that fits does not reach the allocator at all
    M::fail_next = 1;
    CHECK(b.ensure(64) == 0 && b.cap() == 64 && M::fail_next == 1 && d.is(0, 0));
    M::fail_next = 0;
}

void moves_and_swap() {
    Delta d;
    TBuf<int> a;
    CHECK(a.ensure(16) == 0);
    int* const pa = a.get();
    // 4. move construction empties the source and allocates nothing
    TBuf<int> b(std::move(a));
    CHECK(!a && a.get() == nullptr && a.cap() == 0 && b.get() == pa && b.cap() == 16 && d.is(1, 0));
    // move assignment frees the target's old block once and empties the source
    TBuf<int> c;
    CHECK(c.ensure(32) == 0 && d.is(1, 0));
    c = std::move(b);
    CHECK(!b && b.cap() == 0 && c.get() == pa && c.cap() == 16 && d.is(0, 1));
    // into an empty target, from an empty source, and onto itself
    TBuf<int> e;
    e = std::move(c);
    CHECK(!c && e.get() == pa && e.cap() == 16 && d.is(0, 0));
    e = std::move(c);   // (c is empty: e's block is freed)
    CHECK(!e && !c && d.is(0, 1) && M::live == 0);
    CHECK(e.ensure(4) == 0 && d.is(1, 0));
    TBuf<int>& self = e;
    e = std::move(self);
    CHECK(e && e.cap() == 4 && d.is(0, 0));
    // 5. swap exchanges the pointer and the capacity, with an empty buffer too
    TBuf<int> f;
    CHECK(f.ensure(9) == 0 && d.is(1, 0));
    int* const pe = e.get();
    int* const pf = f.get();
    e.swap(f);
    CHECK(e.get() == pf && e.cap() == 9 && f.get() == pe && f.cap() == 4 && d.is(0, 0));
    TBuf<int> g;
    g.swap(e);
    CHECK(!e && e.cap() == 0 && g.get() == pf && g.cap() == 9 && d.is(0, 0));
    // the grow-with-copy of the resident points and the keyframe pool: a local buffer swapped in on success
    {
        TBuf<int> bigger;
        CHECK(bigger.ensure(18) == 0);
        std::memcpy(bigger.get(), g.get(), 9 * sizeof(int));
        g.swap(bigger);
    }   // (the old block leaves with the local)
    CHECK(g.cap() == 18 && d.is(1, 1));
    // 6. reset() frees exactly once, and once only
    g.reset();
    g.reset();
    CHECK(!g && d.is(0, 1));
}   // f and (empty) a, b, c, e, g are destroyed: one free

}  // namespace

int main() {
    reuse_and_growth();
    CHECK(M::live == 0 && M::allocs == M::frees);
    failed_allocation();
    CHECK(M::live == 0 && M::allocs == M::frees);
    const int frees = M::frees;
    moves_and_swap();
    CHECK(M::live == 0 && M::allocs == M::frees && M::frees > frees);
    {   // an array of buffers and a struct of them, as the owners hold them
        struct Owner {
            TBuf<uint8_t> a, b[2];
        };
        Owner* o = new Owner();
        CHECK(o->a.ensure(3) == 0 && o->b[1].ensure(1, 4096) == 0 && o->b[1].cap() == 4096 && M::live == 2);
        delete o;
    }
    // 7. nothing is left
    CHECK(M::live == 0 && M::allocs == M::frees);
    std::printf("allocs %d frees %d live %d\n", M::allocs, M::frees, M::live);
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
