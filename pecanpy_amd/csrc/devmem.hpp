// devmem.hpp -- the one owner of a device (or pinned host) allocation, of a stream, of an event.  Host code only.
//
// A Buf frees what it holds when it goes out of scope, moves but never copies, and hands kernels and argument structs the
// plain pointer `.p`.  Allocation reports the runtime's hipError_t and leaves no sticky error behind: the caller decides
// the error code and the text, or that the failure is no error at all.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <type_traits>

namespace pw {

struct DeviceMem {
    static hipError_t get(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static void put(void *p) { (void)hipFree(p); }
};
struct PinnedMem {
    static hipError_t get(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void put(void *p) { (void)hipHostFree(p); }
};

template <typename T> struct elem_bytes { static constexpr size_t value = sizeof(T); };
template <> struct elem_bytes<void> { static constexpr size_t value = 1; };   // (Buf<void>: sized in bytes)

template <typename T, typename Mem = DeviceMem> struct Buf {
    T *p = nullptr;
    size_t cap = 0;   // elements asked for (0 with p set: the block of a zero-size request)

    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    Buf(Buf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    Buf &operator=(Buf &&o) noexcept {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~Buf() { release(); }

    size_t bytes() const { return cap * elem_bytes<T>::value; }
    // a fresh allocation of n elements in place of whatever was held; a zero-size request still gets a (16-byte) block
    hipError_t alloc(size_t n) {
        release();
        const size_t b = n * elem_bytes<T>::value;
        const hipError_t e = Mem::get((void **)&p, b ? b : 16);
        if (e != hipSuccess) { p = nullptr; (void)hipGetLastError(); return e; }
        cap = n;
        return hipSuccess;
    }
    // room for n elements; grows by a fresh allocation, the contents are not kept
    hipError_t ensure(size_t n) { return n <= cap ? hipSuccess : alloc(n); }
    void release() {
        if (p) Mem::put(p);
        p = nullptr;
        cap = 0;
    }
};

template <typename T> using DevBuf = Buf<T, DeviceMem>;
template <typename T> using PinnedBuf = Buf<T, PinnedMem>;

static_assert(!std::is_copy_constructible<DevBuf<float>>::value && !std::is_copy_assignable<DevBuf<float>>::value, "a Buf has one owner");
static_assert(std::is_nothrow_move_constructible<DevBuf<float>>::value && std::is_nothrow_move_assignable<DevBuf<float>>::value, "a Buf moves");
static_assert(!std::is_copy_constructible<PinnedBuf<void>>::value && std::is_nothrow_move_constructible<PinnedBuf<void>>::value, "pinned too");

// The one owner of a stream or an event: destroyed with it, moves but never copies, and converts to the plain handle wherever
// the runtime or a launch takes one.  create() reports the runtime's hipError_t like Buf::alloc.
struct StreamHandle {
    typedef hipStream_t type;
    static hipError_t make(type *h, unsigned flags) { return hipStreamCreateWithFlags(h, flags); }
    static void destroy(type h) { (void)hipStreamDestroy(h); }
};
struct EventHandle {
    typedef hipEvent_t type;
    static hipError_t make(type *h, unsigned flags) { return hipEventCreateWithFlags(h, flags); }
    static void destroy(type h) { (void)hipEventDestroy(h); }
};

template <typename H> struct Owned {
    typename H::type h = nullptr;

    Owned() = default;
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    Owned(Owned &&o) noexcept : h(o.h) { o.h = nullptr; }
    Owned &operator=(Owned &&o) noexcept {
        if (this != &o) { release(); h = o.h; o.h = nullptr; }
        return *this;
    }
    ~Owned() { release(); }

    operator typename H::type() const { return h; }
    hipError_t create(unsigned flags) { release(); return H::make(&h, flags); }
    void release() {
        if (h) H::destroy(h);
        h = nullptr;
    }
};

using Stream = Owned<StreamHandle>;   // (the handles of this library: hipStreamNonBlocking)
using Event = Owned<EventHandle>;     // (hipEventDefault: timed; hipEventDisableTiming: ordering only)

static_assert(!std::is_copy_constructible<Stream>::value && std::is_nothrow_move_constructible<Stream>::value, "a stream has one owner");
static_assert(!std::is_copy_constructible<Event>::value && std::is_nothrow_move_constructible<Event>::value, "an event has one owner");

}  // namespace pw
