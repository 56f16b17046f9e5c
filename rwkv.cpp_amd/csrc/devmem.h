// devmem.h -- who owns device and pinned host memory: a buffer is a member (or a local) of the type below and is released with its owner.
// Streams, events, graphs and IPC handles are not memory and stay with the code that orders them. Kernel parameter structs take the raw
// pointer (.p); an owner that is destroyed has drained, in its free function, the stream its buffers were used on.
#pragma once
#include <cstddef>
#include <utility>

#include <hip/hip_runtime.h>

namespace rwkvmi {

// `count` elements of T from hipMalloc (DevBuf) or hipHostMalloc(..., hipHostMallocDefault) (PinBuf); move-only.
template <typename T, bool Pinned> struct MemBuf {
    T * p = nullptr;
    size_t count = 0;
    MemBuf() = default;
    MemBuf(const MemBuf &) = delete;
    MemBuf & operator=(const MemBuf &) = delete;
    MemBuf(MemBuf && o) noexcept : p(o.p), count(o.count) { o.p = nullptr; o.count = 0; }
    MemBuf & operator=(MemBuf && o) noexcept {
        if (this != &o) { reset(); p = o.p; count = o.count; o.p = nullptr; o.count = 0; }
        return *this;
    }
    ~MemBuf() { reset(); }
    T * get() const { return p; }
    explicit operator bool() const { return p != nullptr; }
    void reset() {
        if (p) (void) (Pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr; count = 0;
    }
    // releases what it holds, then allocates; a failure leaves it empty
    hipError_t alloc(size_t n) {
        reset();
        const hipError_t e = Pinned ? hipHostMalloc((void **) &p, n * sizeof(T), hipHostMallocDefault) : hipMalloc((void **) &p, n * sizeof(T));
        if (e == hipSuccess) count = n; else p = nullptr;
        return e;
    }
    // a fresh device buffer of host words, copied on `st`
    bool upload(const T * src, size_t n, hipStream_t st) {
        static_assert(!Pinned, "upload fills a device buffer");
        return alloc(n) == hipSuccess && hipMemcpyAsync(p, src, n * sizeof(T), hipMemcpyHostToDevice, st) == hipSuccess;
    }
};
template <typename T> using DevBuf = MemBuf<T, false>;
template <typename T> using PinBuf = MemBuf<T, true>;

// Growing a group of buffers as ONE decision: every new piece is allocated first, and only when all of them exist are the old ones released
// and replaced. On a failure the new pieces are freed, the sticky HIP error is cleared and every buffer is what it was.
//   hipError_t e = grow(want(a, n), want(b, m));        (a count of 0: that buffer stays)
template <typename Buf> struct GrowReq { Buf & buf; size_t count; Buf fresh; };
template <typename Buf> GrowReq<Buf> want(Buf & buf, size_t count) { return GrowReq<Buf>{buf, count, Buf()}; }

template <typename... Req> hipError_t grow(Req &&... reqs) {
    hipError_t e = hipSuccess;
    ((e = (e == hipSuccess && reqs.count) ? reqs.fresh.alloc(reqs.count) : e), ...);
    if (e != hipSuccess) {
        (reqs.fresh.reset(), ...);
        (void) hipGetLastError();
        return e;
    }
    ((reqs.count ? (void) (reqs.buf = std::move(reqs.fresh)) : (void) 0), ...);
    return hipSuccess;
}

// A staged table: a device buffer and pinned staging of the same size and layout, as one owner -- the words of a call, which the host fills
// or reads in the staging, at the Fields of the call's layout (call_layout.h). grow(want(...)) takes it like a MemBuf. The copies are
// asynchronous on `st`: the caller keeps the staging untouched until the stream has passed them.
template <typename T> struct Field;
struct Staged {
    DevBuf<uint8_t> dev;
    PinBuf<uint8_t> pin;
    explicit operator bool() const { return dev.p != nullptr; }
    size_t bytes() const { return dev.count; }
    void reset() { dev.reset(); pin.reset(); }
    // both or neither; a failure leaves it empty
    hipError_t alloc(size_t n) {
        hipError_t e = dev.alloc(n);
        if (e == hipSuccess) e = pin.alloc(n);
        if (e != hipSuccess) reset();
        return e;
    }
    template <typename T> T * h(const Field<T> & f) const { return (T *) (pin.p + f.off); }
    template <typename T> T * d(const Field<T> & f) const { return (T *) (dev.p + f.off); }
    // the bytes [from, to) of the staging to the device, or back
    hipError_t upload(size_t from, size_t to, hipStream_t st) const { return hipMemcpyAsync(dev.p + from, pin.p + from, to - from, hipMemcpyHostToDevice, st); }
    hipError_t fetch(size_t from, size_t to, hipStream_t st) const { return hipMemcpyAsync(pin.p + from, dev.p + from, to - from, hipMemcpyDeviceToHost, st); }
};
// a staged table of one field: `n` rows of T
template <typename T> struct StagedRows : Staged {
    hipError_t alloc(size_t n) { return Staged::alloc(n * sizeof(T)); }
    T * h() const { return (T *) pin.p; }
    T * d() const { return (T *) dev.p; }
    hipError_t upload_rows(size_t from, size_t to, hipStream_t st) const { return Staged::upload(from * sizeof(T), to * sizeof(T), st); }   // rows [from, to)
};

}  // namespace rwkvmi
