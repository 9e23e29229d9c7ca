// The HIP resources a codec or a stream context holds, each owned by the member that names it: device buffers, pinned host blocks,
// events and streams.  None can be copied; each frees what it holds when it goes, so a context is released by deleting it — the
// caller has entered the resources' device and nothing that uses them is in flight.  Each is EMPTY after a failed creation.  Whether
// HIP's last error is cleared then is stated per function: the buffers clear it themselves, the others leave it to their caller,
// which is where the code that creates them on first use has always differed.
// (plain HIP runtime calls only: tools/hostfuzz/codec_res_main.cpp compiles this header against a counting stand-in)
#pragma once
#include <hip/hip_runtime.h>

namespace zpk {

struct NoCopy {
    NoCopy() {}
    NoCopy(const NoCopy&) = delete;
    NoCopy& operator=(const NoCopy&) = delete;
};

// One device buffer (pointer + capacity in bytes).
struct DevBufBase : NoCopy {
    void* p = nullptr; unsigned long long cap = 0;
    ~DevBufBase() { release(); }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    // quiet: exactly `bytes` bytes in place of whatever it held; false: none, the buffer is empty and HIP's last error is cleared
    bool alloc(unsigned long long bytes)
    {
        release();
        if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); p = nullptr; return false; }
        cap = bytes;
        return true;
    }
    // ... for the allocations of one fixed size that are never regrown: made by the first call, kept by every later one
    bool ensure(unsigned long long bytes) { return p || alloc(bytes); }
    void swap(DevBufBase& o) { void* q = p; p = o.p; o.p = q; const unsigned long long k = cap; cap = o.cap; o.cap = k; }
};
template <class T> struct DevBuf : DevBufBase {
    operator T*() const { return (T*)p; }
    template <class U> explicit operator U*() const { return (U*)p; }
};

// One block of pinned host memory that grows, for tables and bytes that travel in one copy.  grow -> the block holds `need` bytes;
// false: no pinned memory (the HIP error is cleared, the block is empty) — what then is the caller's policy.
struct PinBuf : NoCopy {
    unsigned char* p = nullptr; unsigned long long cap = 0;
    ~PinBuf() { release(); }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
    bool grow(unsigned long long need, unsigned flags = hipHostMallocDefault)
    {
        if (need <= cap) return true;
        release();
        const unsigned long long want = need + need / 4 + 4096;
        if (hipHostMalloc((void**)&p, want, flags) != hipSuccess) { (void)hipGetLastError(); p = nullptr; return false; }
        cap = want;
        return true;
    }
};
// ... and one of a fixed size, created on first use: ready -> it exists; false: it does not (HIP's last error is left to the caller)
template <class T> struct PinBlock : NoCopy {
    T* p = nullptr;
    ~PinBlock() { release(); }
    void release() { if (p) (void)hipHostFree((void*)p); p = nullptr; }
    bool ready(unsigned long long bytes, unsigned flags)
    {
        if (p) return true;
        if (hipHostMalloc((void**)&p, bytes, flags) != hipSuccess) { p = nullptr; return false; }
        return true;
    }
    operator T*() const { return p; }
    T* operator->() const { return p; }
};

// An event, created on first use: ready -> hipSuccess when it exists (made now, or by an earlier call), HIP's error when it cannot
// be made (left uncleared).  hipEventDefault makes it with hipEventCreate, any other flags with hipEventCreateWithFlags.
struct Event : NoCopy {
    hipEvent_t e = nullptr;
    ~Event() { if (e) (void)hipEventDestroy(e); }
    hipError_t ready(unsigned flags)
    {
        if (e) return hipSuccess;
        const hipError_t rc = flags == hipEventDefault ? hipEventCreate(&e) : hipEventCreateWithFlags(&e, flags);
        if (rc != hipSuccess) e = nullptr;
        return rc;
    }
    operator hipEvent_t() const { return e; }
};

// A stream, likewise; ready_priority makes it at `priority`
struct Stream : NoCopy {
    hipStream_t s = nullptr;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    hipError_t ready(unsigned flags)
    {
        if (s) return hipSuccess;
        const hipError_t rc = hipStreamCreateWithFlags(&s, flags);
        if (rc != hipSuccess) s = nullptr;
        return rc;
    }
    hipError_t ready_priority(unsigned flags, int priority)
    {
        if (s) return hipSuccess;
        const hipError_t rc = hipStreamCreateWithPriority(&s, flags, priority);
        if (rc != hipSuccess) s = nullptr;
        return rc;
    }
    operator hipStream_t() const { return s; }
};

// A second stream beside a batch's own (created on first use) with the event pair that forks work onto it and joins it back
struct SideStream { Stream s; Event fork, join; };

}  // namespace zpk
