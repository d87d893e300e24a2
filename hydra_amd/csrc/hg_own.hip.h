// The owning types of the library's host code: device memory, pinned memory, a stream, an event.  Each frees
// what it holds when it goes out of scope, so no function and no handle keeps a list of what to free.
#pragma once

// Device memory that frees itself: move-only; alloc(n) makes room for n elements (what it held before is freed first).  Converts to
// the pointer, so it goes where a T* went: kernel arguments, hipMemcpy, pointer arithmetic.
template <class T>
struct DevBuf {
    T* p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) {
            release();
            p = o.p;
            o.p = nullptr;
        }
        return *this;
    }
    ~DevBuf() { release(); }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
    int alloc_bytes(size_t bytes) // for a T with a tail behind it
    {
        release();
        HIP_TRY(hipMalloc(&p, bytes));
        return 0;
    }
    int alloc(size_t n) { return alloc_bytes(n * sizeof(T)); }
    void adopt(T* q) // memory from another device allocator that hipFree releases
    {
        release();
        p = q;
    }
    operator T*() const { return p; }
    T* operator->() const { return p; }
};

// Pinned host memory, the same shape
template <class T>
struct PinBuf {
    T* p = nullptr;
    PinBuf() = default;
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
    PinBuf(PinBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
    PinBuf& operator=(PinBuf&& o) noexcept
    {
        if (this != &o) {
            release();
            p = o.p;
            o.p = nullptr;
        }
        return *this;
    }
    ~PinBuf() { release(); }
    void release()
    {
        if (p) (void)hipHostFree(p);
        p = nullptr;
    }
    int alloc_bytes(size_t bytes)
    {
        release();
        HIP_TRY(hipHostMalloc(&p, bytes));
        return 0;
    }
    int alloc(size_t n) { return alloc_bytes(n * sizeof(T)); }
    operator T*() const { return p; }
    T* operator->() const { return p; }
};

// A stream and an event of their owner's lifetime: created once where the owner is built, never moved
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    int create()
    {
        HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        return 0;
    }
    operator hipStream_t() const { return s; }
};

struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() { if (e) (void)hipEventDestroy(e); }
    int create()
    {
        HIP_TRY(hipEventCreate(&e));
        return 0;
    }
    operator hipEvent_t() const { return e; }
};
