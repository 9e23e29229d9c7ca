// A stand-in for <hip/hip_runtime.h> with only what zpack_amd/csrc/codec_res.h uses, for tools/hostfuzz/codec_res_main.cpp (g++ knows no
// HIP): memory is the host's (so AddressSanitizer sees a double free, a leak or a write past a block), events and streams are small heap
// objects, everything alive is counted, and the k-th creating call can be told to fail.  The last error is sticky until hipGetLastError
// takes it, as HIP's is.
#pragma once
#include <stddef.h>
#include <stdlib.h>

typedef enum { hipSuccess = 0, hipErrorOutOfMemory = 2 } hipError_t;
typedef struct fake_event { int tag; }* hipEvent_t;
typedef struct fake_stream { int tag; }* hipStream_t;
enum { hipHostMallocDefault = 0, hipHostMallocNonCoherent = 0x80000000u >> 1 };
enum { hipEventDefault = 0, hipEventDisableTiming = 2, hipEventReleaseToSystem = 0x40000000 };
enum { hipStreamNonBlocking = 1 };

struct FakeHip {
    long dev = 0, pinned = 0, events = 0, streams = 0;      // alive now
    long creates = 0, fail_at = 0;                          // creating calls so far; the one that fails (1-based, 0: none)
    long calls = 0, cleared = 0, device_waits = 0;          // every call; hipGetLastError calls that took an error; hipDeviceSynchronize calls
    unsigned last_pin_flags = 0, last_event_flags = 0, last_stream_flags = 0; int last_priority = 0, plain_event_creates = 0;
    hipError_t pending = hipSuccess;
    long live() const { return dev + pinned + events + streams; }
    bool fails() { calls++; creates++; if (creates == fail_at) { pending = hipErrorOutOfMemory; return true; } return false; }
};
inline FakeHip& fake_hip() { static FakeHip f; return f; }

inline hipError_t hipGetLastError() { FakeHip& f = fake_hip(); f.calls++; const hipError_t e = f.pending; if (e != hipSuccess) f.cleared++; f.pending = hipSuccess; return e; }
inline hipError_t hipDeviceSynchronize() { fake_hip().calls++; fake_hip().device_waits++; return hipSuccess; }
inline hipError_t hipMalloc(void** p, size_t bytes) { FakeHip& f = fake_hip(); if (f.fails()) return hipErrorOutOfMemory; *p = malloc(bytes ? bytes : 1); f.dev++; return hipSuccess; }
inline hipError_t hipFree(void* p) { FakeHip& f = fake_hip(); f.calls++; free(p); f.dev--; return hipSuccess; }
inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned flags)
{
    FakeHip& f = fake_hip();
    f.last_pin_flags = flags;
    if (f.fails()) return hipErrorOutOfMemory;
    *p = malloc(bytes ? bytes : 1); f.pinned++;
    return hipSuccess;
}
inline hipError_t hipHostFree(void* p) { FakeHip& f = fake_hip(); f.calls++; free(p); f.pinned--; return hipSuccess; }
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags)
{
    FakeHip& f = fake_hip();
    f.last_event_flags = flags;
    if (f.fails()) return hipErrorOutOfMemory;
    *e = (hipEvent_t)malloc(sizeof(fake_event)); f.events++;
    return hipSuccess;
}
inline hipError_t hipEventCreate(hipEvent_t* e) { fake_hip().plain_event_creates++; return hipEventCreateWithFlags(e, hipEventDefault); }
inline hipError_t hipEventDestroy(hipEvent_t e) { FakeHip& f = fake_hip(); f.calls++; free(e); f.events--; return hipSuccess; }
inline hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned flags, int priority)
{
    FakeHip& f = fake_hip();
    f.last_stream_flags = flags; f.last_priority = priority;
    if (f.fails()) return hipErrorOutOfMemory;
    *s = (hipStream_t)malloc(sizeof(fake_stream)); f.streams++;
    return hipSuccess;
}
inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned flags) { return hipStreamCreateWithPriority(s, flags, 0); }
inline hipError_t hipStreamDestroy(hipStream_t s) { FakeHip& f = fake_hip(); f.calls++; free(s); f.streams--; return hipSuccess; }
