// Buf<T, Mem>: the one owner of a device or pinned allocation.  Move-only; cap() is in elements of T.
// Mem is a policy of two static functions,
//     error alloc(void** p, size_t bytes);   (a value-initialised error is success, as hipSuccess is)
//     void  free(void* p);
// so this header names no HIP symbol (the policies are beside Ctx, orbgpu_ctx.h) and compiles with a plain host
// compiler (tests/cpp_buf).  The destructor frees and does not choose a device: whoever deletes the owning object
// makes its device current and synchronises its stream first.
#pragma once
#include <algorithm>
#include <cstddef>
#include <utility>

namespace orbgpu {

template <class T, class Mem>
class Buf {
    T* p_ = nullptr;
    size_t cap_ = 0;

public:
    using Err = decltype(Mem::alloc((void**)nullptr, (size_t)0));
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    Buf(Buf&& o) noexcept : p_(o.p_), cap_(o.cap_) {
        o.p_ = nullptr;
        o.cap_ = 0;
    }
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) {
            reset();
            swap(o);
        }
        return *this;
    }
    ~Buf() { reset(); }

    T* get() const { return p_; }
    size_t cap() const { return cap_; }
    explicit operator bool() const { return p_ != nullptr; }
    void swap(Buf& o) noexcept {
        std::swap(p_, o.p_);
        std::swap(cap_, o.cap_);
    }
    void reset() {
        if (p_) Mem::free(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    // Room for n elements.  Allocated and large enough: nothing happens and the pointer stays (launch arguments and
    // graph keys hold it).  Otherwise the old block is freed first and max(n, floor) elements allocated; contents
    // are not kept.  On failure the buffer is empty.
    Err ensure(size_t n, size_t floor = 0) {
        if (p_ && n <= cap_) return Err{};
        reset();
        const size_t want = std::max(n, floor);
        void* q = nullptr;
        const Err e = Mem::alloc(&q, want * sizeof(T));
        if (e != Err{}) return e;
        p_ = static_cast<T*>(q);
        cap_ = want;
        return e;
    }
};

}  // namespace orbgpu
