// zpack_amd/csrc/codec_res.h, the header the codec compiles, under ASan + UBSan against a counting stand-in for the HIP runtime
// (tools/hostfuzz/fakehip): every owning type created, used, regrown and destroyed with nothing left alive and nothing freed twice; the
// creation failing at every call of such a run — the object is empty, HIP's last error is cleared by the types that clear it and left
// by those that leave it to their caller, everything else still goes cleanly —; an object destroyed untouched; ready() twice.
// Built and run by tools/hostfuzz/run_codec_res.sh
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <initializer_list>
#include "codec_res.h"
using namespace zpk;
typedef unsigned long long u64;

#define CHECK(x) do { if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); exit(1); } } while (0)

// the codec's grow() (zpk_codec.hip) without its codec: the device-wide wait before a regrow, need + need / 4 + 4096, then need + 256
static bool grow(DevBufBase& b, u64 need)
{
    if (need <= b.cap) return true;
    if (b.p) { (void)hipDeviceSynchronize(); b.release(); }
    return b.alloc(need + need / 4 + 4096) || b.alloc(need + 256);
}
// ... and the stream contexts' dgrow_keep (zpk_stream.inc): a new block, the first `keep` bytes carried over, the old one released behind
static bool grow_keep(DevBuf<unsigned char>& b, u64 need, u64 keep)
{
    if (need <= b.cap) return true;
    DevBuf<unsigned char> nb;
    if (!nb.alloc(need + need / 2 + 4096) && !nb.alloc(need + 256)) return false;
    if (b && keep) memcpy(nb, b, keep);
    b.swap(nb);
    return true;
}

// What a codec and a stream context hold, by kind
struct Holder {
    DevBuf<unsigned> counters; DevBuf<unsigned char> staging, kept;
    PinBuf table; PinBlock<unsigned char> pin; PinBlock<u64> words;
    Event ev, timer; Stream st; SideStream side;
};

// One run: every creation in turn, in the way the codec makes it.  A creation that fails (the stand-in's fail_at) must leave its object
// empty and the last error cleared (cleared = true) or pending (false); the run goes on with the rest.  -> the creating calls it made
static long run(long fail_at)
{
    FakeHip& f = fake_hip();
    f = FakeHip(); f.fail_at = fail_at;
    long failed = 0;
    {
        Holder h;
        auto step = [&](bool ok, bool empty_now, bool clears) {
            if (ok) { CHECK(f.pending == hipSuccess); return; }
            failed++;
            CHECK(empty_now);
            CHECK(clears ? f.pending == hipSuccess : f.pending != hipSuccess);      // who clears HIP's last error: the buffers do, the others' callers
            (void)hipGetLastError();
        };
        bool ok;
        // DevBuf: the exact allocation, twice; the grow policy (a refused first size is tried again with less slack), a regrow; the carrying grow
        ok = h.counters.ensure(96);             step(ok, !h.counters && h.counters.cap == 0, true);
        const long before = f.creates;
        if (ok) { CHECK(h.counters.ensure(96) && h.counters.cap == 96 && f.creates == before); memset(h.counters, 0x11, 96); }
        {
            const long c0 = f.creates, cl0 = f.cleared;
            ok = grow(h.staging, 1000);
            if (f.creates == c0 + 2) { failed++; CHECK(ok && h.staging.cap == 1256 && f.cleared == cl0 + 1 && f.pending == hipSuccess); }    // the first size was refused: the slack goes
            else CHECK(ok && h.staging.cap == 1000 + 250 + 4096);
            memset(h.staging, 0x22, h.staging.cap);
            CHECK(grow(h.staging, 500) && f.creates <= c0 + 2 && f.device_waits == 0);                                                 // fits: nothing happens
            const long c1 = f.creates;
            ok = grow(h.staging, 100000);                                                                                               // a regrow: the wait, the release, the new block
            CHECK(f.device_waits == 1);
            if (f.creates == c1 + 2) { failed++; CHECK(ok && h.staging.cap == 100256); }
            else CHECK(ok && h.staging.cap == 100000 + 25000 + 4096);
            memset(h.staging, 0x33, h.staging.cap);
        }
        for (const u64 need : { (u64)64, (u64)1 << 20 }) {                                        // the second carries the first's 64 bytes over
            const long c0 = f.creates, cl0 = f.cleared, dev0 = f.dev;
            CHECK(grow_keep(h.kept, need, need == 64 ? 0 : 64) && h.kept && f.dev == dev0 + (need == 64 ? 1 : 0));        // (the old block has left)
            if (f.creates == c0 + 2) { failed++; CHECK(h.kept.cap == need + 256 && f.cleared == cl0 + 1 && f.pending == hipSuccess); }
            else CHECK(h.kept.cap == need + need / 2 + 4096);
            if (need == 64) memset(h.kept, 0x44, h.kept.cap);
            else { for (int i = 0; i < 64; i++) CHECK(((unsigned char*)h.kept)[i] == 0x44); memset(h.kept, 0x45, h.kept.cap); }
        }
        // PinBuf: grows, fits, regrows (the old block released first); flags are the caller's
        ok = h.table.grow(300);                 step(ok, !h.table.p && h.table.cap == 0, true);
        if (ok) { CHECK(h.table.cap == 300 + 75 + 4096 && f.last_pin_flags == hipHostMallocDefault); memset(h.table.p, 0x55, h.table.cap); const long c = f.creates; CHECK(h.table.grow(4000) && f.creates == c); }
        ok = h.table.grow(1 << 16, hipHostMallocNonCoherent);   step(ok, !h.table.p && h.table.cap == 0, true);
        if (ok) { CHECK(h.table.cap == 65536 + 16384 + 4096 && f.last_pin_flags == hipHostMallocNonCoherent); memset(h.table.p, 0x66, h.table.cap); }
        // PinBlock: made once, the flags are the caller's, the error is the caller's to clear
        ok = h.pin.ready(4096, hipHostMallocNonCoherent);       step(ok, !h.pin, false);
        if (ok) { CHECK(f.last_pin_flags == hipHostMallocNonCoherent); memset(h.pin, 0x77, 4096); const long c = f.creates; CHECK(h.pin.ready(4096, hipHostMallocNonCoherent) && f.creates == c); }
        ok = h.words.ready(64, hipHostMallocDefault);           step(ok, !h.words, false);
        if (ok) { h.words[7] = 7; CHECK(f.last_pin_flags == hipHostMallocDefault); }
        // Event: with flags, and the plain creation of the timers; ready() twice creates once
        ok = h.ev.ready(hipEventDisableTiming | hipEventReleaseToSystem) == hipSuccess;           step(ok, !h.ev, false);
        if (ok) { CHECK(f.last_event_flags == (hipEventDisableTiming | hipEventReleaseToSystem) && f.plain_event_creates == 0); const long c = f.creates; CHECK(h.ev.ready(hipEventDisableTiming) == hipSuccess && f.creates == c && f.events == 1); }
        const int plain = f.plain_event_creates;
        ok = h.timer.ready(hipEventDefault) == hipSuccess;      step(ok, !h.timer, false);
        CHECK(f.plain_event_creates == plain + 1);
        // Stream: with flags; at a priority (the side stream of a decode batch), with its two events
        ok = h.st.ready(hipStreamNonBlocking) == hipSuccess;    step(ok, !h.st, false);
        if (ok) { CHECK(f.last_stream_flags == hipStreamNonBlocking); const long c = f.creates; CHECK(h.st.ready(hipStreamNonBlocking) == hipSuccess && f.creates == c && f.streams == 1); }
        ok = h.side.s.ready_priority(hipStreamNonBlocking, 3) == hipSuccess;                      step(ok, !h.side.s, false);
        if (ok) CHECK(f.last_priority == 3);
        ok = h.side.fork.ready(hipEventDisableTiming) == hipSuccess;                              step(ok, !h.side.fork, false);
        ok = h.side.join.ready(hipEventDisableTiming) == hipSuccess;                              step(ok, !h.side.join, false);
        // what failed can be made by the next call that needs it (created on first use, again)
        f.fail_at = 0;
        CHECK(h.counters.ensure(96) && h.pin.ready(4096, hipHostMallocDefault) && h.ev.ready(hipEventDisableTiming) == hipSuccess && h.st.ready(hipStreamNonBlocking) == hipSuccess);
        CHECK(f.live() > 0);
    }
    CHECK(f.live() == 0 && f.dev == 0 && f.pinned == 0 && f.events == 0 && f.streams == 0);       // the holder is gone: nothing is alive
    CHECK(fail_at == 0 ? failed == 0 : failed == 1);
    return f.creates;
}

int main()
{
    const long full = run(0);
    printf("full: %ld creating calls, every type created, used, regrown and destroyed, nothing alive at the end\n", full);
    long runs = 0;
    for (long k = 1; k <= full; k++) { (void)run(k); runs++; }
    printf("failing: the creation refused at each of the calls 1..%ld in turn: the object empty, the error cleared by the buffers and left by the others, the rest destroyed cleanly\n", runs);
    {
        FakeHip& f = fake_hip();
        f = FakeHip();
        { Holder h; DevBuf<void> v; PinBuf p; PinBlock<volatile int> q; Event e; Stream s; SideStream x; (void)h; }
        CHECK(f.calls == 0 && f.live() == 0);
        printf("untouched: default-constructed objects are destroyed without one call\n");
    }
    {
        FakeHip& f = fake_hip();
        f = FakeHip();
        {
            Event e; Stream s; PinBlock<int> p; DevBuf<int> d;
            for (int i = 0; i < 2; i++) CHECK(e.ready(hipEventDisableTiming) == hipSuccess && s.ready(hipStreamNonBlocking) == hipSuccess && p.ready(16, hipHostMallocDefault) && d.ensure(16));
            CHECK(f.creates == 4 && f.live() == 4);
            const hipEvent_t e0 = e; const hipStream_t s0 = s; int* const p0 = p; int* const d0 = d;
            CHECK(e.ready(hipEventDefault) == hipSuccess && (hipEvent_t)e == e0 && (hipStream_t)s == s0 && (int*)p == p0 && (int*)d == d0);
        }
        CHECK(f.creates == 4 && f.live() == 0);
        printf("twice: ready() and ensure() a second time create nothing and keep what the first made\n");
    }
    printf("ok\n");
    return 0;
}
