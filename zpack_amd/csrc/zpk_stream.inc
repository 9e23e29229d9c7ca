// zpk_stream.inc — streaming triple over the device codec (included by zpk_codec.hip).
//
// Stands where the reference keeps library streaming contexts + the XXH3 state
// (lib/zpack_stream.c:4-28, lib/zpack_read.c:515-640, lib/zpack_write.c:461-685).
//
// READ (round 3: bounded host memory, output while input is still arriving).  A decode stream owns three device buffers — the
// compressed entry (comp_size), its output (uncomp_size) and a resume record — and NO host staging: every step appends the caller's
// chunk to the device copy, runs one resumable decode step (k_lz4_stream / k_zstd_stream, one wave: every complete LZ4F block /
// Zstandard block the bytes so far hold is decoded, the positions + — Zstandard — repeat offsets, table state and LDS image are parked
// in the record, lz4_wave.h Lz4Resume / zstd_wg.h ZstdResume), and hands back whatever output exists beyond what the caller already
// has.  The first output bytes of a 512 MiB entry leave after its first block, not after its last input byte, and the host never
// holds more than the caller's own two windows.  The XXH3 of the whole output is computed on the device when the frame is complete
// (lib/zpack_read.c:631-637: the verdict arrives with the last byte).  Stored entries take the same route (decode = nothing).
// WRITE (round 4: output while input is still arriving, bounded device memory).  The plaintext is appended to a device buffer of a
// few MiB; whenever more than a step's worth has arrived, the complete 512 KiB pieces in it are compressed — runs of blocks of the
// entry's ONE frame (round 5: the frame header goes out in front of the first piece, zpk_cstream_finish closes the frame; round 4 made
// every piece a frame of its own), up to eight of them side by side as one encode batch — packed back to back and handed out; the
// XXH3 of the whole plaintext is kept as a running state on the device (zpk_cs_state).  The reference's streaming writer keeps one
// library frame open across calls too (lib/zpack_write.c:477-574); pieces of 512 KiB lose nothing against that here, because this encoder's
// match window is 64 KiB anyway.  First output after the first 512 KiB of input; the device holds <= ~5 MiB of plaintext.

struct zpk_stream_rec {                          // written by the stream kernels, read back after every step
    i32 rc; u32 fired;
    u64 produced;                                // output bytes that are final
    u64 hash;
    Lz4Resume lz4;
};

__global__ __launch_bounds__(64) void k_lz4_stream(const u8* __restrict__ in, u64 in_len, u8* out, u64 cap, zpk_stream_rec* __restrict__ rec)
{
    const int lane = lane_id();
    __shared__ Lz4WaveShared shw;
    Watchdog wd; wd.arm(in_len + cap, ZPK_WATCHDOG_RETRY_SCALE);
    SeqStats stt = {};
    Lz4Resume rs;
    rs.ip_off = uni64(rec->lz4.ip_off); rs.op_off = uni64(rec->lz4.op_off); rs.in_blocks = uni(rec->lz4.in_blocks);
    rs.frame_ip_off = uni64(rec->lz4.frame_ip_off); rs.frame_op_off = uni64(rec->lz4.frame_op_off); rs.nframes = uni(rec->lz4.nframes);
    const DecodeOut o = lz4f_decode_wave(shw, wd, stt, in, in_len, in, in + in_len, out, cap, lane, &rs);
    lane0_guard();
    if (lane == 0) { rec->rc = o.rc; rec->fired = wd.fired ? 1u : 0u; rec->produced = o.produced; rec->lz4 = rs; }
}

__global__ __launch_bounds__(ZSTD_WG_THREADS, 3) void k_zstd_stream(const u8* __restrict__ in, u64 in_len, u8* out, u64 cap, zpk_stream_rec* __restrict__ rec,
                                                                 ZstdResume* __restrict__ zr, u8* __restrict__ lit, int final)
{
    const int lane = lane_id();
    __shared__ ZstdShared sh;
    if (threadIdx.x == 0) { sh.defaults_built = 0; sh.huf_valid = 0; }
    __syncthreads();
    Watchdog wd; wd.arm(in_len + cap, ZPK_WATCHDOG_RETRY_SCALE);
    const DecodeOut o = zstd_decode_wave<false>(sh, wd, in, in_len, out, cap, lit, lane, nullptr, nullptr, zr, final != 0);
    lane0_guard();
    if (lane == 0) { rec->rc = o.rc; rec->fired = wd.fired ? 1u : 0u; rec->produced = o.produced; }
}

// XXH3 of the finished output, into the record
__global__ __launch_bounds__(64) void k_stream_hash(const u8* __restrict__ out, u64 len, zpk_stream_rec* __restrict__ rec)
{
    const int lane = lane_id();
    const u64 h = xxh3_64_wave(out, len, lane);
    lane0_guard();
    if (lane == 0) rec->hash = h;
}

// What ONLY the bounded block-parallel steps use (round 5; dstream_fast_* below).  DsFastEntry is the state of the entry being read: cleared
// as a whole between entries (dstream_clear); DsFast adds the buffers, which stay.
struct DsFastEntry {
    u64 pend_len;                                // bytes in DsFast::pend
    u64 in_total;                                // compressed bytes taken so far
    int hdr, indep, has_cs; u64 content;         // the frame header is parsed (its size); LZ4: independent blocks; content size
    u64 T, hist, ghashed;                        // output bytes of the finished steps; history bytes in front of the device window; 64 KiB groups hashed
    u64 avail, given, delivered;                 // the size of the last step's output, what the caller has of it; output bytes handed out in all
    // Zstandard steps: the window, the repeat offsets and the last block with a Huffman tree travel from step to step
    u64 window, fcs, hist_cap;
    u32 reps[3];
    u32 tree_len;                                // bytes in DsFast::tree
    u32 tab_mode[3], tab_len[3]; u8 tab_desc[3][FZ_TABDESC];   // host: what governs the three sequence tables (Repeat_Mode blocks of later steps build them again)
};
struct DsFast : DsFastEntry {
    u8* pend; u64 pend_cap;                      // host: compressed bytes that are not decoded yet (from a block boundary on)
    DevBuf<u8> d_f;                              // device: everything an LZ4 step needs (a fixed ~40 MiB, dstream_fast_layout); the scratch of a Zstandard step
    DevBuf<u8> d_fo;                             // device, Zstandard: [history | a step's output] + what persists between steps (XXH3 state)
    PinBlock<u8> h_out;                          // host, pinned: the output of the last step
    u8* tree;                                    // host: the most recent block whose literals section carries a tree (Treeless blocks of later steps read it)
};
struct zpk_dstream {
    zpk_codec* c;                                // the codec of the CURRENT call (a stream outlives codecs: never touched by reset / destroy)
    int device;                                  // where the buffers below live
    DevBuf<u8> d_in; u64 in_len;                 // device: the compressed bytes so far
    DevBuf<u8> d_out;                            // device: the output slot (uncomp_size)
    DevBuf<u8> d_aux;                            // device: zpk_stream_rec | ZstdResume | literal scratch
    u64 avail, out_pos;                          // output bytes that exist on the device / that the caller has
    int complete, status;                        // the frame is decoded and hashed; the verdict to give with the last byte
    // Small chunks are gathered on the host first (round 4): the reference's own test feeds 16-byte windows (tests/read_archive.c:38-82),
    // and a kernel launch + two copies + a synchronisation per 16 bytes is three orders of magnitude of overhead.  A step is taken when
    // ZPK_DS_GATHER bytes are waiting, when the entry's last byte has arrived, or when the caller has nothing to hand out otherwise —
    // bounded host memory (ZPK_DS_GATHER), at most one launch per ZPK_DS_GATHER bytes of input.
    u8* h_in; u64 h_len;                         // host: compressed bytes taken from the caller, not yet on the device
    u64 launches, calls;                         // (diagnostics: decode steps launched / calls served)
    int fast;                                    // 0 undecided, 1 the bounded steps are running, -1 not for this entry (the windowless step)
    DsFast f;
};

// ---- streaming XXH3 of the plaintext: the accumulators of the long-input path between steps ----
struct zpk_cs_state { u64 acc[8]; u64 hash; };
__global__ __launch_bounds__(64) void k_xxh3s_init(zpk_cs_state* __restrict__ st)
{
    const int lane = lane_id();
    Xxh3Wave w; w.init(lane);
    if (lane < 4) { st->acc[2 * lane] = w.a0; st->acc[2 * lane + 1] = w.a1; }
}
// `nblocks` whole 1 KiB blocks that are known NOT to hold the input's last byte (XXH3 treats the last block differently)
__global__ __launch_bounds__(64) void k_xxh3s_blocks(zpk_cs_state* __restrict__ st, const u8* __restrict__ p, u64 nblocks)
{
    const int lane = lane_id();
    Xxh3Wave w; w.init(lane);
    w.a0 = st->acc[2 * (lane & 3)]; w.a1 = st->acc[2 * (lane & 3) + 1];
    for (u64 b = 0; b < nblocks; b++) w.block(ld128(p + (b << 10) + 16 * lane));
    lane0_guard();
    if (lane < 4) { st->acc[2 * lane] = w.a0; st->acc[2 * lane + 1] = w.a1; }
}
// the rest: `rem` >= 1 bytes at p (the 64 bytes in front of p are the bytes that precede them in the input), `total` bytes in all
__global__ __launch_bounds__(64) void k_xxh3s_finish(zpk_cs_state* __restrict__ st, const u8* __restrict__ p, u64 rem, u64 total)
{
    const int lane = lane_id();
    u64 h;
    if (total <= 240) h = xxh3_64_wave(p, total, lane);                 // (never stepped: everything is still here)
    else {
        Xxh3Wave w; w.init(lane);
        w.a0 = st->acc[2 * (lane & 3)]; w.a1 = st->acc[2 * (lane & 3) + 1];
        const u64 nb = (rem - 1) >> 10;
        for (u64 b = 0; b < nb; b++) w.block(ld128(p + (b << 10) + 16 * lane));
        h = uni64(w.finish(p + (nb << 10), (u32)(((rem - 1) - (nb << 10)) >> 6), p + rem, total, lane));
    }
    lane0_guard();
    if (lane == 0) st->hash = h;
}

#define ZPK_CS_PIECES 8u                         // pieces compressed side by side in one step
#define ZPK_CS_CARRY 64u                         // bytes kept in front of the buffered plaintext (the XXH3's last stripe may reach back)
struct zpk_cstream {
    zpk_codec* c;
    int device;
    DevBuf<u8> d_in; u64 in_len;                 // device: [carry][plaintext not yet compressed]
    DevBuf<u8> d_out;                            // device: the frames not yet handed out, back to back
    DevBuf<u8> d_slots;                          // device: bound-sized output slots of one step
    DevBuf<u8> d_aux;                            // device: zpk_cs_state | descriptors | results | offsets
    u64 out_len, out_pos;
    u64 total_in, total_out;                     // of the entry so far (total_out: compressed bytes produced)
    u32 method; i32 level; int configured, steps;
    int framed;                                  // the frame header of an entry that goes out in pieces has been written
};

// device buffer of at least `need` bytes that keeps its first `keep` bytes.  Sizes here derive from what the caller says about the
// entry: nothing may wrap (a wrapped size would allocate a few bytes and hand the kernels a huge capacity).
static int dgrow_keep(zpk_codec* c, DevBuf<u8>& b, u64 need, u64 keep)
{
    if (need <= b.cap) return ZPK_OK;
    if (need > ZPK_STREAM_MAX_BYTES || keep > b.cap) return ZPK_E_NOMEM;
    DevBuf<u8> nb;                                                                   // (the old block leaves with it, behind the copy)
    if (!nb.alloc(need + need / 2 + 4096) && !nb.alloc(need + 256)) return ZPK_E_NOMEM;
    if (b && keep && hipMemcpyAsync(nb, b, keep, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) return ZPK_E_LAUNCH;
    if (b) (void)hipStreamSynchronize(c->stream);
    b.swap(nb);
    return ZPK_OK;
}

extern "C" {

int zpk_dstream_create(zpk_codec* c, zpk_dstream** out)
{
    if (!c || !out) return ZPK_E_INVALID;
    zpk_dstream* s = new (std::nothrow) zpk_dstream();                                // (no member has an initialiser: all zero, the buffers empty)
    if (!s) return ZPK_E_NOMEM;
    s->c = c; s->device = c->device; *out = s;
    return ZPK_OK;
}

// (device memory belongs to a device, not to a codec: the codec a stream last worked with may be gone by now)
static void dstream_release(zpk_dstream* s)
{
    if (s && s->h_in) { free(s->h_in); s->h_in = nullptr; s->h_len = 0; }
    if (s && s->f.pend) { free(s->f.pend); s->f.pend = nullptr; s->f.pend_len = s->f.pend_cap = 0; }
    if (s && s->f.tree) { free(s->f.tree); s->f.tree = nullptr; s->f.tree_len = 0; }
    if (!s || !(s->d_in || s->d_out || s->d_aux || s->f.d_f || s->f.h_out || s->f.d_fo)) return;
    if (hipSetDevice(s->device) != hipSuccess) return;
    s->f.h_out.release();
    s->f.d_f.release(); s->f.d_fo.release();
    // (every step ends with a synchronisation of the stream it ran on, so nothing is in flight on these buffers: no device-wide wait —
    // hipFree itself orders the release behind outstanding work)
    s->d_in.release(); s->d_out.release(); s->d_aux.release();
}

// The state of the entry being read, cleared in one place.  A replay (the entry's bytes once more through the windowless step, after
// ZPK_DS_RESTART) keeps what the caller already has of the entry — f.delivered, the count of calls — and leaves the bounded steps
// (fast = -1); a reset drops those too and leaves the route undecided.  Every buffer stays either way.
static void dstream_clear(zpk_dstream* s, bool replay)
{
    const u64 delivered = replay ? s->f.delivered : 0;
    s->in_len = 0; s->avail = 0; s->out_pos = 0; s->complete = 0; s->status = 0; s->h_len = 0; s->launches = 0;
    if (!replay) s->calls = 0;
    static_cast<DsFastEntry&>(s->f) = DsFastEntry();
    s->f.delivered = delivered;
    s->fast = replay ? -1 : 0;
}

// the codec the NEXT step decodes with (a stream may outlive codecs): device memory belongs to a device — moving on releases it
void zpk_dstream_bind(zpk_dstream* s, zpk_codec* c)
{
    if (!s || !c) return;
    if (s->device != c->device) dstream_release(s);
    s->c = c; s->device = c->device;
}

void zpk_dstream_reset(zpk_dstream* s)
{
    if (!s) return;
    dstream_clear(s, false);
    // a stream that has carried a large entry gives the device memory back between entries
    if (s->d_in.cap + s->d_out.cap + s->f.d_f.cap + s->f.d_fo.cap > (64ull << 20)) dstream_release(s);
}

void zpk_dstream_destroy(zpk_dstream* s) { if (s) { dstream_release(s); delete s; } }

// diagnostics: bytes of device memory the stream holds right now
uint64_t zpk_dstream_device_bytes(const zpk_dstream* s) { return s ? s->d_in.cap + s->d_out.cap + s->d_aux.cap + s->f.d_f.cap + s->f.d_fo.cap : 0; }

// diagnostics: decode steps launched / calls served since the last reset
void zpk_dstream_counters(const zpk_dstream* s, uint64_t* launches, uint64_t* calls)
{
    if (launches) *launches = s ? s->launches : 0;
    if (calls) *calls = s ? s->calls : 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Block-parallel streaming in BOUNDED memory (round 5).  The path above keeps the whole entry — compressed and decoded — on the device
// and decodes it with one wave (80 MB/s): an entry larger than the device fails where the reference, which writes into the caller's
// window (lib/zpack_read.c:560-620), succeeds.  A large entry (>= ZPK_DS_FAST_MIN compressed bytes) that is ONE plain LZ4 frame — what
// the reference writer produces: 64 KiB blocks, no checksums — goes in steps of up to 64 blocks instead: the host keeps the compressed
// bytes that are not decoded yet (at most a step's worth + the caller's window), finds the complete blocks among them, and a step
// decodes them side by side (lz4_pj.h: parse, references, pointer doubling, gather) behind the last 128 KiB of output, which stay on the
// device as history; the step's output comes back into a pinned buffer and is handed out; the XXH3 runs along in sections
// (xxh3_span.h).  Device memory: ~40 MiB whatever the entry's size.  The reader pulls no new input while a step's output is waiting
// (zpk_dstream_wants_input).  ANYTHING else — another header flavour, a second frame, a skippable frame, a damaged or truncated
// block, sizes that disagree — is not decided here: the step answers ZPK_DS_RESTART, the caller feeds the entry's bytes so far again
// (zpk_dstream_replay) and the stream goes on above, where the verdicts are; the bytes handed out so far are not handed out again.
//
// A step (stream_plan.h has every rule that is not a launch): intake of the caller's bytes — header, once — the complete blocks among
// the pending bytes — go / wait / RESTART — buffers (the first step allocates) — upload and the kernel pipeline up to the gather (what
// the two codecs differ in) — the XXH3 so far — the output home and the history carry — ONE synchronisation — commit and hand-out.
static_assert(sizeof(zpk_span) <= FS_SMALL && sizeof(zpk_stream_rec) <= FS_SMALL && sizeof(zpk_decode_desc) == FZ_DESC_BYTES && FS_SRC_SLACK == ZPK_SRC_SLACK,
              "stream_plan.h lays the steps' device blocks out with these sizes");
static_assert(F_FIRST_MIN == ZPK_PJ_MIN_BLOCKS && FZ_FIRST_MIN == ZPK_ZPJ_MIN_BLOCKS, "the first step's minimum is the block-parallel readers'");

static int dstream_fast_deliver(zpk_dstream* s, uint8_t* out, size_t out_cap, size_t* produced, int* done)
{
    const u64 left = s->f.avail - s->f.given;
    const u64 give = out_cap < left ? out_cap : left;
    if (give) memcpy(out, s->f.h_out + s->f.given, give);
    s->f.given += give; s->f.delivered += give; *produced = give;
    if (s->complete && s->f.given == s->f.avail) { *done = 1; return s->status; }
    return 0;
}

// The caller's bytes join the pending ones; a call that finds output waiting (or the entry complete) only hands out.
// -> true: *rc is the call's answer; false: the step goes on
static bool dstream_fast_intake(zpk_dstream* s, uint64_t comp_size, const uint8_t* in, size_t in_size, size_t* consumed,
                                uint8_t* out, size_t out_cap, size_t* produced, int* done, int* rc)
{
    const StreamIntake it = stream_intake(comp_size, s->f.in_total, in_size);
    if ((*rc = it.rc) != 0) return true;
    *consumed = it.take;
    if (it.take) {
        const u64 cap = stream_pend_cap(s->f.pend_len, s->f.pend_cap, it.take);
        if (cap != s->f.pend_cap) {
            u8* nb = (u8*)realloc(s->f.pend, cap);
            if (!nb) { *rc = 10; return true; }
            s->f.pend = nb; s->f.pend_cap = cap;
        }
        memcpy(s->f.pend + s->f.pend_len, in, it.take);
        s->f.pend_len += it.take; s->f.in_total += it.take;
    }
    s->calls++;
    if (s->f.given < s->f.avail || s->complete) { *rc = dstream_fast_deliver(s, out, out_cap, produced, done); return true; }
    return false;
}

// the frame header is parsed: its `hdr` bytes leave the pending ones
static void dstream_fast_header_done(zpk_dstream* s, int hdr)
{
    s->f.hdr = hdr;
    memmove(s->f.pend, s->f.pend + hdr, s->f.pend_len - (u64)hdr);
    s->f.pend_len -= (u64)hdr;
}

// the device block `need` bytes large and the pinned output buffer: nothing of this entry lives there before its first step, which allocates
static int dstream_fast_buffers(zpk_dstream* s, DevBuf<u8>& dev, u64 need)
{
    if (dev.cap < need) {
        if (s->f.T != 0) return ZPK_DS_RESTART;
        if (!dev.alloc(need)) return ZPK_DS_RESTART;
    }
    if (!s->f.h_out.ready(F_HOST_OUT, hipHostMallocDefault)) { (void)hipGetLastError(); return ZPK_DS_RESTART; }
    return 0;
}

// What the shared parts of a step work on, and the step's scope guard: the asynchronous copies of a step name host memory of the step —
// hf, hh, span here, the block tables of its function — so from the first enqueue (arm) to the step's own synchronisation (sync) every
// way out waits for the stream.  Declared BEHIND every local a copy names: it leaves first.  Costs nothing where a step succeeds.
struct FastStep {
    hipStream_t st; bool armed;
    u8* d_out; u8* d_tmp; u64 hist_cap;          // the window [history | step output], the temporary of the carry, the history's capacity
    u64* d_part; zpk_span* d_span; u64* d_hash; u64* d_state; zpk_stream_rec* rec; u32* flags;
    zpk_span span; u64 hh; u32 hf[64];           // host ends of the step's small copies
    explicit FastStep(hipStream_t stream) : st(stream), armed(false), hh(0) {}
    FastStep(const FastStep&) = delete;
    void arm() { armed = true; }
    hipError_t sync() { armed = false; return hipStreamSynchronize(st); }
    ~FastStep() { if (armed) (void)hipStreamSynchronize(st); }
};

// Pointer doubling over blocks [b0, b1) of nt: `look` rounds, then a look whether the last one still moved anything (LZ4 looks every
// F_LOOK rounds, Zstandard every FZ_LOOK: launch counts and synchronisation points of the two steps as they were measured).
// -> 0, 24, or ZPK_DS_RESTART (a damaged block; rounds that never settle)
static int dstream_jump_rounds(FastStep& F, u32* S, const PjBlock* B, u32 b0, u32 b1, u32 nt, u32 jgrid, u32 look)
{
    for (u32 r0 = 0; r0 < PJ_MAX_ROUNDS; r0 += look) {
        const u32 r1 = r0 + look < PJ_MAX_ROUNDS ? r0 + look : PJ_MAX_ROUNDS;
        for (u32 r = r0; r < r1; r++) hipLaunchKernelGGL(k_pj_jump, dim3(jgrid), dim3(256), 0, F.st, S, B, b0, b1, nt, F.flags, r);
        hipError_t e = hipMemcpyAsync(F.hf, F.flags, (PJ_ROUND0 + PJ_MAX_ROUNDS) * 4, hipMemcpyDeviceToHost, F.st);
        if (e == hipSuccess) e = hipStreamSynchronize(F.st);
        if (e != hipSuccess) return 24;
        if (F.hf[PJ_ERR]) return ZPK_DS_RESTART;
        if (!F.hf[PJ_ROUND0 + r1 - 1]) break;
        if (r1 == PJ_MAX_ROUNDS) return ZPK_DS_RESTART;
    }
    return 0;
}

// XXH3 of everything produced so far (stream_hash_plan): whole 64 KiB groups as they become final, the rest with the end; an entry that
// ends in its first step is hashed in one launch.  With the end the hash is on its way to F.hh.
static hipError_t dstream_hash_so_far(zpk_dstream* s, FastStep& F, u64 T_new, bool end)
{
    const StreamHash h = stream_hash_plan(s->f.T, s->f.hist, T_new, s->f.ghashed, end);
    if (h.one_shot) {
        hipLaunchKernelGGL(k_stream_hash, dim3(1), dim3(64), 0, F.st, (const u8*)F.d_out, T_new, F.rec);
        return hipMemcpyAsync(&F.hh, &F.rec->hash, 8, hipMemcpyDeviceToHost, F.st);
    }
    if (h.chain) {
        const u8* const virt = F.d_out - h.virt_back;                                    // position p of the output lies at virt + p
        u64* const part_v = F.d_part - h.part_back;
        F.span.off = 0; F.span.len = T_new; F.span.part_base = 0;
        const hipError_t e = hipMemcpyAsync(F.d_span, &F.span, sizeof(F.span), hipMemcpyHostToDevice, F.st);
        if (e != hipSuccess) return e;
        if (h.partials)
            hipLaunchKernelGGL(k_xxh3_partials, dim3((u32)((h.g_to - h.g_from + 3) / 4)), dim3(256), 0, F.st, virt, (const zpk_span*)F.d_span, 1u, h.g_from, h.g_to, part_v);
        hipLaunchKernelGGL(k_xxh3_chain, dim3(1), dim3(64), 0, F.st, virt, (const zpk_span*)F.d_span, (const u64*)part_v, F.d_hash, F.d_state, h.b_from, h.b_to, h.last);
        s->f.ghashed = h.ghashed_new;
    }
    return end ? hipMemcpyAsync(&F.hh, F.d_hash, 8, hipMemcpyDeviceToHost, F.st) : hipSuccess;
}

// The step's output home, `flag_bytes` of the flags with it; the last hist_cap bytes stay as the next step's history (stream_carry);
// then the step's ONE synchronisation.  e: what the enqueues before have answered.  -> 0 or 24
static int dstream_home_and_carry(zpk_dstream* s, zpk_codec* c, FastStep& F, hipError_t e, u64 step_out, bool end, u64 flag_bytes)
{
    if (e == hipSuccess && step_out) e = hipMemcpyAsync(s->f.h_out, F.d_out + s->f.hist, step_out, hipMemcpyDeviceToHost, F.st);
    if (e == hipSuccess) e = hipMemcpyAsync(F.hf, F.flags, flag_bytes, hipMemcpyDeviceToHost, F.st);
    if (e == hipSuccess) {
        const StreamCarry k = stream_carry(s->f.hist, step_out, F.hist_cap, end);
        if (k.move) {
            e = hipMemcpyAsync(F.d_tmp, F.d_out + k.from, k.keep, hipMemcpyDeviceToDevice, F.st);
            if (e == hipSuccess) e = hipMemcpyAsync(F.d_out, F.d_tmp, k.keep, hipMemcpyDeviceToDevice, F.st);
        }
        s->f.hist = k.hist_new;
    }
    if (e == hipSuccess) e = F.sync();
    if (e != hipSuccess) { snprintf(c->err, sizeof(c->err), "stream step: %s", hipGetErrorString(e)); return 24; }
    return 0;
}

// the step is final: its `q` compressed bytes leave the pending ones, its output waits in the pinned buffer; the verdict with the end
// (lib/zpack_read.c:631-637: it arrives with the last byte)
static int dstream_commit_and_deliver(zpk_dstream* s, const FastStep& F, u64 T_new, u64 step_out, u64 q, bool end, uint64_t hash,
                                      uint8_t* out, size_t out_cap, size_t* produced, int* done)
{
    s->f.T = T_new; s->f.avail = step_out; s->f.given = 0; s->launches++;
    memmove(s->f.pend, s->f.pend + q, s->f.pend_len - q);
    s->f.pend_len -= q;
    if (end) { s->complete = 1; s->status = stream_verdict(F.hh, hash); }
    return dstream_fast_deliver(s, out, out_cap, produced, done);
}

// -> a zpack_result, or ZPK_DS_RESTART
static int dstream_fast_lz4(zpk_dstream* s, zpk_codec* c, uint64_t comp_size, uint64_t uncomp_size, uint64_t hash,
                            const uint8_t* in, size_t in_size, size_t* consumed, uint8_t* out, size_t out_cap, size_t* produced, int* done)
{
    int rc = 0;
    if (dstream_fast_intake(s, comp_size, in, in_size, consumed, out, out_cap, produced, done, &rc)) return rc;
    const bool all_in = s->f.in_total == comp_size;
    const u8* const P = s->f.pend;
    // ---- the frame header, once ----
    if (!s->f.hdr) {
        const int hdr = lz4_single_header(P, s->f.pend_len, &s->f.indep, &s->f.has_cs, &s->f.content);
        if (hdr < 0 || (hdr == 0 && all_in)) return ZPK_DS_RESTART;
        if (hdr == 0) return 0;
        dstream_fast_header_done(s, hdr);
    }
    // ---- the complete blocks among the pending bytes ----
    PjBlock tab[F_BLOCKS];
    u64 q = 0; bool end = false;
    const int found = lz4_stream_blocks(P, s->f.pend_len, tab, F_BLOCKS, &q, &end);
    if (found < 0) return ZPK_DS_RESTART;
    const u32 nb = (u32)found;
    const StreamGo go = stream_go(end, nb, F_BLOCKS, F_FIRST_MIN, s->f.T, all_in, q == s->f.pend_len);
    if (go != STREAM_RUN) return go == STREAM_RESTART ? ZPK_DS_RESTART : 0;
    // ---- one step ----
    if (hipSetDevice(c->device) != hipSuccess) return 24;
    const FastLayout L = dstream_fast_layout();
    if ((rc = dstream_fast_buffers(s, s->f.d_f, L.size)) != 0) return rc;
    u8* const d_f = s->f.d_f;
    u8* const d_in = d_f + L.in; u32* const S = (u32*)(d_f + L.S); PjBlock* const B = (PjBlock*)(d_f + L.blocks);
    FastStep F(c->stream);
    F.d_out = d_f + L.out; F.d_tmp = d_f + L.tmp; F.hist_cap = F_HIST; F.d_part = (u64*)(d_f + L.part); F.d_span = (zpk_span*)(d_f + L.span);
    F.d_hash = (u64*)(d_f + L.hash); F.d_state = (u64*)(d_f + L.state); F.rec = (zpk_stream_rec*)(d_f + L.rec); F.flags = (u32*)(d_f + L.flags);
    hipStream_t st = F.st;
    u64 step_out = 0;
    hipError_t e = hipSuccess;
    if (nb) {
        F.arm();
        e = hipMemcpyAsync(d_in, P, q, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(B, tab, nb * sizeof(PjBlock), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemsetAsync(F.flags, 0, 256, st);
        if (e != hipSuccess) return 24;
        hipLaunchKernelGGL(k_pj_parse, dim3(nb), dim3(64), 0, st, (const u8*)d_in, q, B, nb, (u64*)(d_f + L.recs), (u32*)(d_f + L.masks), F.flags);
        hipLaunchKernelGGL(k_pj_scan, dim3(1), dim3(64), 0, st, B, nb, F.flags, (u32)s->f.hist);
        e = hipMemcpyAsync(F.hf, F.flags, 16, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return 24;
        const u64 total = ((u64)F.hf[PJ_TOTAL + 1] << 32) | F.hf[PJ_TOTAL];
        if (F.hf[PJ_ERR] || total < s->f.hist || total - s->f.hist > F_OUT) return ZPK_DS_RESTART;
        step_out = total - s->f.hist;
        if (s->f.T + step_out > uncomp_size) return ZPK_DS_RESTART;                      // more than the entry may hold: BUFFER_TOO_SMALL is not ours to say
        hipLaunchKernelGGL(k_pj_init, dim3(nb), dim3(256), 0, st, (const PjBlock*)B, 0u, nb, (const u64*)(d_f + L.recs), (const u32*)(d_f + L.masks), S, total, F.flags, s->f.indep);
        if (step_out) {
            const u32 jgrid = (u32)((step_out + 1023) / 1024), ggrid = (u32)((total - (s->f.hist & ~3ull) + 1023) / 1024);
            if ((rc = dstream_jump_rounds(F, S, B, 0u, nb, nb, jgrid, F_LOOK)) != 0) return rc;
            hipLaunchKernelGGL(k_pj_gather, dim3(ggrid), dim3(256), 0, st, (const u32*)S, (const PjBlock*)B, 0u, nb, nb, (const u8*)d_in, q, F.d_out, F.flags);
        }
    }
    const u64 T_new = s->f.T + step_out;
    if (end && s->f.has_cs && s->f.content != T_new) return ZPK_DS_RESTART;
    F.arm();
    e = dstream_hash_so_far(s, F, T_new, end);
    if ((rc = dstream_home_and_carry(s, c, F, e, step_out, end, 4)) != 0) return rc;
    if (nb && F.hf[PJ_ERR]) return ZPK_DS_RESTART;                                       // (the history was moved: harmless, the replay starts over)
    return dstream_commit_and_deliver(s, F, T_new, step_out, q, end, hash, out, out_cap, produced, done);
}

// The same for ONE plain Zstandard frame (ZSTD_compressCCtx: no checksum, no dictionary; a window of at most 8 MiB): steps of up to 64
// blocks (zstd_pj.h: sequences and literals of all blocks side by side, then references / pointer doubling / gather in chunks of 16
// blocks) behind the frame's window of output, which stays on the device as history.  From step to step travel: the window, the three
// repeat offsets, the running XXH3 and — on the host — the last block whose literals carry a Huffman tree (Treeless blocks of later
// steps read its description: it goes up again in front of the step's blocks) and the table descriptions in force.
static int dstream_fast_zstd(zpk_dstream* s, zpk_codec* c, uint64_t comp_size, uint64_t uncomp_size, uint64_t hash,
                             const uint8_t* in, size_t in_size, size_t* consumed, uint8_t* out, size_t out_cap, size_t* produced, int* done)
{
    int rc = 0;
    if (dstream_fast_intake(s, comp_size, in, in_size, consumed, out, out_cap, produced, done, &rc)) return rc;
    const bool all_in = s->f.in_total == comp_size;
    const u8* const P = s->f.pend;
    // ---- the frame header, once ----
    if (!s->f.hdr) {
        u64 window = 0, fcs = ~0ull;
        const int hdr = zpj_parse_frame_header(P, s->f.pend_len, FZ_MAX_WLOG, &window, &fcs);
        if (hdr < 0 || (hdr == 0 && all_in)) return ZPK_DS_RESTART;
        if (hdr == 0) return 0;
        if (!fz_window_ok(window)) return ZPK_DS_RESTART;
        s->f.window = window; s->f.fcs = fcs; s->f.hist_cap = fz_hist_cap(window);
        s->f.reps[0] = 1; s->f.reps[1] = 4; s->f.reps[2] = 8; s->f.tree_len = 0;
        for (int k = 0; k < 3; k++) { s->f.tab_mode[k] = 3; s->f.tab_len[k] = 0; }
        dstream_fast_header_done(s, hdr);
    }
    // ---- the complete blocks among the pending bytes; table entry 0 = the inherited tree block (if any) ----
    std::vector<ZpjBlock> tab;
    const u32 tb = s->f.tree_len ? 1u : 0u;                    // table index of the step's first block
    // the device copy of a step: [3 x FZ_TABDESC: the table descriptions earlier steps left in force][the tree block][the step's blocks]
    const u64 tree_at = 3ull * FZ_TABDESC;
    const u64 in_base = tree_at + (s->f.tree_len ? (((u64)s->f.tree_len + 63) & ~63ull) : 0);
    ZpjTabs tabs; for (int k = 0; k < 3; k++) { tabs.mode[k] = s->f.tab_mode[k]; tabs.off[k] = (u32)(k * FZ_TABDESC); }
    u64 q = 0, slots = 0, lit_total = 0;
    u32 nb = 0, tree = s->f.tree_len ? 0u : ZPJ_NONE, new_tree = ZPJ_NONE;
    bool end = false;
    try {
        if (s->f.tree_len) {
            ZpjBlock T; u32 tl = 0; u64 tt = 0;
            if (zpj_parse_block(s->f.tree, s->f.tree_len, tree_at, T, &tl, &tt) != 1 || T.type != 2 || T.lit_type != 2) return ZPK_DS_RESTART;
            T.type = ZPJ_TREE_ONLY; T.nseq = 0;
            tab.push_back(T);
        }
        while (nb < FZ_BLOCKS && !end) {
            ZpjBlock B; u32 last = 0; u64 total = 0;
            const int pr = zpj_parse_block(P + q, s->f.pend_len - q, in_base + q, B, &last, &total, &tabs);
            if (pr < 0) return ZPK_DS_RESTART;
            if (pr == 0) break;
            if (B.type == 2 && B.lit_type == 2) new_tree = nb;
            if (!zpj_place_block(B, tb + nb, tree, slots, lit_total)) return ZPK_DS_RESTART;
            tab.push_back(B);
            nb++; q += total;
            if (last) end = true;
        }
    } catch (...) { return 10; }
    const StreamGo go = stream_go(end, nb, FZ_BLOCKS, FZ_FIRST_MIN, s->f.T, all_in, q == s->f.pend_len);
    if (go != STREAM_RUN) return go == STREAM_RESTART ? ZPK_DS_RESTART : 0;
    // ---- one step ----
    if (hipSetDevice(c->device) != hipSuccess) return 24;
    const u32 nt = tb + nb;                                     // table entries
    const u64 in_len = in_base + q, arena_off = (in_len + 64 + 255) & ~255ull, src_total = arena_off + lit_total;
    const FzLayout L = dstream_fz_layout(nt, slots, src_total, s->f.hist_cap);
    if ((rc = dstream_fast_buffers(s, s->f.d_fo, L.fo_need)) != 0) return rc;
    if (s->f.d_f.cap < L.size) {                                  // the scratch holds nothing between steps: any step may grow it
        if (!s->f.d_f.alloc(fz_scratch_alloc(L.size))) return ZPK_DS_RESTART;
    }
    u8* const d_f = s->f.d_f; u8* const d_fo = s->f.d_fo;
    u8* const d_in = d_f + L.in;
    ZpjBlock* const ZB = (ZpjBlock*)(d_f + L.zb); PjBlock* const B = (PjBlock*)(d_f + L.pb);
    std::vector<zpk_decode_desc> items; std::vector<u32> list; std::vector<PjBlock> hb;
    try {
        items.assign(nt, zpk_decode_desc()); hb.assign(nt, PjBlock());
        memset(items.data(), 0, nt * sizeof(zpk_decode_desc)); memset(hb.data(), 0, nt * sizeof(PjBlock));
        for (u32 b = 0; b < nt; b++) {
            if (tab[b].type == 2 && tab[b].lit_type >= 2) tab[b].lit_ref = (u32)(arena_off + tab[b].lit_base);
            if (tab[b].type != 2 || tab[b].nseq == 0) continue;
            items[b].src_offset = tab[b].hdr_off; items[b].comp_size = 3ull + tab[b].size;
            items[b].dst_offset = 8ull * tab[b].seq_base; items[b].dst_capacity = 8ull * tab[b].nseq; items[b].method = ZPK_METHOD_ZSTD;
            items[b].uncomp_size = (u64)tab[b].tab_off[0] | ((u64)tab[b].tab_off[1] << 32);     // (k_zstd_fse_blocks: inherited table descriptions)
            items[b].expect_hash = (u64)tab[b].tab_off[2] | ((u64)tab[b].tab_modes << 32);
            list.push_back(b);
        }
    } catch (...) { return 10; }
    u32 hflags[64]; memset(hflags, 0, sizeof(hflags));
    hflags[ZPJ_CNT + C_ZSTD] = (u32)list.size();
    FastStep F(c->stream);
    F.d_out = d_fo + L.out; F.d_tmp = d_fo + L.tmp; F.hist_cap = s->f.hist_cap; F.d_part = (u64*)(d_f + L.part); F.d_span = (zpk_span*)(d_fo + L.p_span);
    F.d_hash = (u64*)(d_fo + L.p_hash); F.d_state = (u64*)(d_fo + L.p_state); F.rec = (zpk_stream_rec*)(d_fo + L.p_rec); F.flags = (u32*)(d_fo + L.p_flags);
    hipStream_t st = F.st;
    u32* const flags = F.flags;
    F.arm();
    hipError_t e = hipMemcpyAsync(d_in, s->f.tab_desc, 3 * FZ_TABDESC, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && s->f.tree_len) e = hipMemcpyAsync(d_in + tree_at, s->f.tree, s->f.tree_len, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && q) e = hipMemcpyAsync(d_in + in_base, P, q, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(ZB, tab.data(), nt * sizeof(ZpjBlock), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(B, hb.data(), nt * sizeof(PjBlock), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_f + L.desc, items.data(), nt * sizeof(zpk_decode_desc), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && !list.empty()) e = hipMemcpyAsync(d_f + L.list, list.data(), list.size() * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(d_f + L.state, 0, (L.recs - L.state), st);
    if (e == hipSuccess) e = hipMemcpyAsync(flags, hflags, sizeof(hflags), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return 24;
    u32* const state = (u32*)(d_f + L.state); u32* const rep_out = (u32*)(d_f + L.rep);
    if (!list.empty()) {
        const u32 rows = (u32)list.size();
        const u32 grid = (rows + ZF_ROWS - 1) / ZF_ROWS < ZF_GRID_MAX ? (rows + ZF_ROWS - 1) / ZF_ROWS : ZF_GRID_MAX;
        hipLaunchKernelGGL(k_zstd_fse_blocks, dim3(grid), dim3(64), 0, st, (const u8*)d_in, (const zpk_decode_desc*)(d_f + L.desc), (const u32*)(d_f + L.list),
                           flags + ZPJ_CNT, (u64*)(d_f + L.recs), state, rep_out, in_len);
    }
    hipLaunchKernelGGL(k_zpj_lit, dim3(nt), dim3(64), 0, st, d_in, src_total, arena_off, (const ZpjBlock*)ZB, nt, flags);
    hipLaunchKernelGGL(k_zpj_reps, dim3(1), dim3(64), 0, st, ZB, nt, (const u32*)state, (const u32*)rep_out, flags, s->f.reps[0], s->f.reps[1], s->f.reps[2]);
    hipLaunchKernelGGL(k_zpj_pos, dim3(nt), dim3(256), 0, st, (const ZpjBlock*)ZB, B, nt, (const u64*)(d_f + L.recs), (u64*)(d_f + L.pos), (u32*)(d_f + L.masks), flags);
    hipLaunchKernelGGL(k_pj_scan, dim3(1), dim3(64), 0, st, B, nt, flags, (u32)s->f.hist);
    e = hipMemcpyAsync(F.hf, flags, sizeof(F.hf), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(hb.data(), B, nt * sizeof(PjBlock), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return 24;
    const u64 total = ((u64)F.hf[PJ_TOTAL + 1] << 32) | F.hf[PJ_TOTAL];
    if (F.hf[PJ_ERR] || total < s->f.hist || total - s->f.hist > FZ_OUT) return ZPK_DS_RESTART;
    const u64 step_out = total - s->f.hist;
    if (s->f.T + step_out > uncomp_size) return ZPK_DS_RESTART;
    // references, pointer doubling, gather: FZ_CHUNK blocks at a time (the references of a chunk are all the scratch this takes)
    for (u32 b0 = tb; b0 < nt; b0 += FZ_CHUNK) {
        const u32 b1 = b0 + FZ_CHUNK < nt ? b0 + FZ_CHUNK : nt;
        const u64 lo = hb[b0].out_off, hi = b1 < nt ? hb[b1].out_off : total;
        if (hi == lo) continue;
        u32* const Sv = (u32*)(d_f + L.S) - lo;               // S[i] for the chunk's positions only
        e = hipMemsetAsync(flags + PJ_ROUND0, 0, PJ_MAX_ROUNDS * 4, st);
        if (e != hipSuccess) return 24;
        hipLaunchKernelGGL(k_zpj_init, dim3(b1 - b0), dim3(256), 0, st, (const ZpjBlock*)ZB, (const PjBlock*)B, b0, nt, (const u64*)(d_f + L.recs), (const u64*)(d_f + L.pos),
                           (const u32*)(d_f + L.masks), Sv, total, flags);
        const u32 jgrid = (u32)((hi - lo + 1023) / 1024), ggrid = (u32)((hi - (lo & ~3ull) + 1023) / 1024);
        if ((rc = dstream_jump_rounds(F, Sv, B, b0, b1, nt, jgrid, FZ_LOOK)) != 0) return rc;
        hipLaunchKernelGGL(k_pj_gather, dim3(ggrid), dim3(256), 0, st, (const u32*)Sv, (const PjBlock*)B, b0, b1, nt, (const u8*)d_in, src_total, F.d_out, flags);
    }
    const u64 T_new = s->f.T + step_out;
    if (end && s->f.fcs != ~0ull && s->f.fcs != T_new) return ZPK_DS_RESTART;
    e = dstream_hash_so_far(s, F, T_new, end);
    if ((rc = dstream_home_and_carry(s, c, F, e, step_out, end, sizeof(F.hf))) != 0) return rc;
    if (F.hf[PJ_ERR]) return ZPK_DS_RESTART;
    // ---- what travels on the host ----
    s->f.reps[0] = F.hf[ZPJ_REPS]; s->f.reps[1] = F.hf[ZPJ_REPS + 1]; s->f.reps[2] = F.hf[ZPJ_REPS + 2];
    for (int k = 0; k < 3; k++) {                                // table descriptions this step put in force: kept for Repeat_Mode blocks to come
        s->f.tab_mode[k] = tabs.mode[k];
        if (tabs.mode[k] != 3 && tabs.off[k] >= in_base) {
            const u64 at = tabs.off[k] - in_base, n = q - at < FZ_TABDESC ? q - at : (u64)FZ_TABDESC;
            memcpy(s->f.tab_desc[k], P + at, n); s->f.tab_len[k] = (u32)n;
        }
    }
    if (new_tree != ZPJ_NONE) {                                  // the step's last block with a tree: kept for the Treeless blocks to come
        const ZpjBlock& TB = tab[tb + new_tree];
        const u64 at = TB.hdr_off - in_base, len = 3ull + TB.size;
        if (!s->f.tree && !(s->f.tree = (u8*)malloc(ZPJ_BLOCK + 64))) return 10;
        memcpy(s->f.tree, P + at, len); s->f.tree_len = (u32)len;
    }
    return dstream_commit_and_deliver(s, F, T_new, step_out, q, end, hash, out, out_cap, produced, done);
}

// 1: the next step wants input; 0: it only has output to hand out (bounded memory: the reader pulls nothing meanwhile)
int zpk_dstream_wants_input(const zpk_dstream* s)
{
    if (!s || s->fast != 1) return 1;
    return (s->f.given < s->f.avail || s->complete) ? 0 : 1;
}

// after ZPK_DS_RESTART: the entry's first bytes again (first = 1 with the first piece), through the windowless step, nothing handed out;
// when all bytes the stream had taken are back the stream goes on where the caller is.  Returns a zpack_result (a verdict may come up here).
int zpk_dstream_replay(zpk_dstream* s, uint32_t method, uint64_t comp_size, uint64_t uncomp_size, uint64_t hash, const uint8_t* in, size_t in_size, int first)
{
    if (!s) return 21;
    if (first) dstream_clear(s, true);
    size_t consumed = 0, produced = 0; int done = 0;
    // what the caller already has is not handed out again (dstream_hand_out skips f.delivered bytes; they are the same bytes: blocks the
    // bounded steps decoded are regular)
    return zpk_dstream_step(s, method, comp_size, uncomp_size, hash, in, in_size, &consumed, nullptr, 0, &produced, &done);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The windowless step: the caller's chunk joins the entry's bytes on the device (small ones are gathered on the host until a step is
// worth a launch), one resumable decode step over everything that is there, the verdict once everything that can be known is known;
// nothing to do once the entry is complete.
// -> 0: go on to the hand-out; anything else is the call's answer
static int dstream_windowless_step(zpk_dstream* s, zpk_codec* c, uint32_t method, uint64_t comp_size, uint64_t uncomp_size, uint64_t hash,
                                   const uint8_t* in, size_t in_size, size_t* consumed)
{
    const u64 aux_need = 256 + sizeof(ZstdResume) + ZSTD_LIT_SCRATCH;
    if (!s->complete) {
        // comp_size / uncomp_size come from the archive's CDR, unverified: every size below is derived from bytes that have actually
        // arrived or actually been produced, never from those two alone — a header that claims 2^64 - 1 bytes costs nothing, an entry
        // that really is larger than the device can hold fails with MALLOC_FAILED (hipMalloc refuses), like the reference's realloc
        if (comp_size < s->in_len + s->h_len) return 21;
        if (comp_size > ZPK_STREAM_MAX_BYTES) return 10; /* ZPACK_ERROR_MALLOC_FAILED */
        s->calls++;
        // ---- the caller's chunk: small ones are gathered on the host until a step is worth a launch ----
        // (the resume record is cleared by the entry's FIRST device step — decided here, before the gather branch below moves bytes into
        // in_len: a first call of a few bytes followed by a large one used to arrive at its first launch with in_len != 0, keep the
        // previous entry's record and resume in the middle of nowhere)
        const bool fresh = s->launches == 0;
        const u64 want_all = comp_size - s->in_len - s->h_len;
        const u64 take_all = in_size < want_all ? in_size : want_all;
        *consumed = take_all;
        const bool last_byte_here = s->in_len + s->h_len + take_all == comp_size;
        const u8* up = in; u64 up_len = take_all;                             // what goes to the device in this call
        if (s->h_len && take_all >= ZPK_DS_GATHER) {                          // a large chunk behind gathered bytes: those go up first
            if (dgrow_keep(c, s->d_in, s->in_len + s->h_len + take_all + 64, s->in_len) != ZPK_OK) return 10;
            if (hipMemcpyAsync(s->d_in + s->in_len, s->h_in, s->h_len, hipMemcpyHostToDevice, c->stream) != hipSuccess) return 24;
            if (hipStreamSynchronize(c->stream) != hipSuccess) return 24;
            s->in_len += s->h_len; s->h_len = 0;
        } else if (take_all < ZPK_DS_GATHER) {
            if (!s->h_in && !(s->h_in = (u8*)malloc(2 * ZPK_DS_GATHER))) return 10;
            memcpy(s->h_in + s->h_len, in, take_all);                        // (h_len < ZPK_DS_GATHER here, take_all < ZPK_DS_GATHER: fits)
            s->h_len += take_all;
            if (s->h_len < ZPK_DS_GATHER && !last_byte_here) return 0;       // not worth a launch yet: the bytes are kept
            up = s->h_in; up_len = s->h_len;
        }
        const u64 take = up_len;
        if (dgrow_keep(c, s->d_in, s->in_len + take + 64, s->in_len) != ZPK_OK) return 10;
        if (dgrow_keep(c, s->d_aux, aux_need, 0) != ZPK_OK) return 10;
        zpk_stream_rec* rec = (zpk_stream_rec*)s->d_aux;
        ZstdResume* zr = (ZstdResume*)(s->d_aux + 256);
        u8* lit = s->d_aux + 256 + sizeof(ZstdResume);
        hipError_t e = hipSuccess;
        if (fresh) e = hipMemsetAsync(s->d_aux, 0, 256 + __builtin_offsetof(ZstdResume, lds), c->stream);      // no resume point yet
        if (e == hipSuccess && take) e = hipMemcpyAsync(s->d_in + s->in_len, up, take, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) return 24;
        s->in_len += take;
        if (up == s->h_in) { if (hipStreamSynchronize(c->stream) != hipSuccess) return 24; s->h_len = 0; }      // the gather buffer is free again
        s->launches++;
        const bool all_in = s->in_len == comp_size;
        zpk_stream_rec h; memset(&h, 0, sizeof(h));
        if (method == ZPK_METHOD_NONE) {
            // lib/zpack_read.c:539-560: the bytes pass through; uncomp_size of them count
            if (uncomp_size > comp_size) return 18; /* ZPACK_ERROR_FILE_SIZE_INVALID */
            if (hipStreamSynchronize(c->stream) != hipSuccess) return 24;        // the bytes below are read back on another stream
            h.rc = all_in ? D_OK : D_TRUNCATED;
            h.produced = s->in_len < uncomp_size ? s->in_len : uncomp_size;
        } else {
            // The output slot grows with what the frame PRODUCES (first 8 MiB, then doubling, never beyond uncomp_size): a step that
            // runs out of room is run again from its resume record in the larger slot (both decoders resume in front of a block).
            for (;;) {
                u64 cap_now = s->d_out.cap >= 64 ? s->d_out.cap - 64 : 0;
                if (cap_now > uncomp_size) cap_now = uncomp_size;
                if (cap_now == 0 && uncomp_size) {
                    const u64 first = uncomp_size < (8ull << 20) ? uncomp_size : (8ull << 20);
                    if (dgrow_keep(c, s->d_out, first + 64, 0) != ZPK_OK) return 10;
                    continue;
                }
                if (!s->d_out && dgrow_keep(c, s->d_out, 64, 0) != ZPK_OK) return 10;      // (an empty entry: still a buffer to point at)
                if (method == ZPK_METHOD_LZ4) hipLaunchKernelGGL(k_lz4_stream, dim3(1), dim3(64), 0, c->stream, (const u8*)s->d_in, s->in_len, s->d_out, cap_now, rec);
                else hipLaunchKernelGGL(k_zstd_stream, dim3(1), dim3(ZSTD_WG_THREADS), 0, c->stream, (const u8*)s->d_in, s->in_len, s->d_out, cap_now, rec, zr, lit, all_in ? 1 : 0);
                e = hipMemcpyAsync(&h, rec, sizeof(h), hipMemcpyDeviceToHost, c->stream);
                if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
                if (e != hipSuccess) { snprintf(c->err, sizeof(c->err), "stream step: %s", hipGetErrorString(e)); return 24; }
                // (LZ4: a frame boundary that falls exactly on a slot smaller than the entry reads as the reference's `avail_out == 0`
                // exit — D_OK with input left over; the caller's real capacity is uncomp_size, so the slot grows and the step goes on)
                const bool short_ok = method == ZPK_METHOD_LZ4 && h.rc == D_OK && h.produced >= cap_now && cap_now < uncomp_size;
                if ((h.rc != D_DST_FULL && !short_ok) || cap_now >= uncomp_size) break;
                u64 bigger = cap_now < (1ull << 45) ? 2 * cap_now : cap_now;
                if (bigger > uncomp_size) bigger = uncomp_size;
                const u64 keep = h.produced < cap_now ? h.produced : cap_now;            // history for the blocks to come
                if (bigger <= cap_now || dgrow_keep(c, s->d_out, bigger + 64, keep) != ZPK_OK) return 10;
            }
        }
        const u8* const body = method == ZPK_METHOD_NONE ? s->d_in : s->d_out;
        s->avail = h.produced < uncomp_size ? h.produced : uncomp_size;
        // ---- verdicts: the one-shot mapping (lib/zpack_read.c:384-388, :421-450), once everything that can be known is known ----
        int status = 0;
        bool finished = false;
        if (h.rc == D_OK && all_in) finished = true;
        else if (h.rc == D_OK || h.rc == D_TRUNCATED) {
            if (all_in) {                        // every input byte is here and the frame is still not complete
                if (method == ZPK_METHOD_LZ4) status = h.produced < uncomp_size ? 17 /* FILE_INCOMPLETE */ : 12 /* BUFFER_TOO_SMALL */;
                else status = 13; /* DECOMPRESS_FAILED */
            }
        }
        else if (h.rc == D_DST_FULL) status = method == ZPK_METHOD_LZ4 ? 12 : 13;
        else status = 13;
        if (status) { s->complete = 1; s->status = status; return status; }
        if (finished) {
            // (lib/zpack_read.c:556,579,609: the streaming reader hashes the bytes it PRODUCED — a frame that ends short of uncomp_size
            // fails the comparison on those, where the one-shot reader hashes its whole buffer)
            hipLaunchKernelGGL(k_stream_hash, dim3(1), dim3(64), 0, c->stream, body, s->avail, rec);
            e = hipMemcpyAsync(&h, rec, sizeof(h), hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) return 24;
            s->complete = 1;
            s->status = stream_verdict(h.hash, hash); /* ZPACK_ERROR_FILE_HASH_MISMATCH: with the last byte, the data stays */
        }
    }
    return 0;
}

// whatever output of the windowless step exists beyond what the caller has
// (after a restart out of the bounded steps the caller already has f.delivered bytes: they are skipped as they come into being)
static int dstream_hand_out(zpk_dstream* s, uint32_t method, uint8_t* out, size_t out_cap, size_t* produced, int* done)
{
    if (s->out_pos < s->f.delivered) s->out_pos = s->f.delivered < s->avail ? s->f.delivered : s->avail;
    const u8* const body = method == ZPK_METHOD_NONE ? s->d_in : s->d_out;
    const u64 left = s->avail - s->out_pos;
    const u64 give = out_cap < left ? out_cap : left;
    if (give) {
        if (hipMemcpy(out, body + s->out_pos, give, hipMemcpyDeviceToHost) != hipSuccess) return 24;
    }
    s->out_pos += give; *produced = give;
    if (s->complete && s->out_pos == s->avail) { *done = 1; return s->status; }   /* hash verdict arrives with the last byte */
    return 0;
}

int zpk_dstream_step(zpk_dstream* s, uint32_t method, uint64_t comp_size, uint64_t uncomp_size, uint64_t hash,
                     const uint8_t* in, size_t in_size, size_t* consumed, uint8_t* out, size_t out_cap, size_t* produced, int* done)
{
    if (!s || !consumed || !produced || !done) return 21; /* ZPACK_ERROR_STREAM_INVALID */
    *consumed = 0; *produced = 0; *done = 0;
    zpk_codec* c = s->c;
    if (!c) return 24;
    if (method != ZPK_METHOD_NONE && method != ZPK_METHOD_ZSTD && method != ZPK_METHOD_LZ4) return 19; /* ZPACK_ERROR_COMP_METHOD_INVALID */
    CodecLock lk(c);
    if (hipSetDevice(c->device) != hipSuccess) return 24; /* ZPACK_ERROR_NOT_AVAILABLE: never a CPU fallback */
    if (s->fast == 0) s->fast = ((method == ZPK_METHOD_LZ4 || method == ZPK_METHOD_ZSTD) && comp_size >= ZPK_DS_FAST_MIN && c->opt.dec_split_min != ~0ull) ? 1 : -1;
    if (s->fast == 1) {
        const int frc = method == ZPK_METHOD_LZ4 ? dstream_fast_lz4(s, c, comp_size, uncomp_size, hash, in, in_size, consumed, out, out_cap, produced, done)
                                                 : dstream_fast_zstd(s, c, comp_size, uncomp_size, hash, in, in_size, consumed, out, out_cap, produced, done);
        if (frc == ZPK_DS_RESTART) { *consumed = 0; *produced = 0; *done = 0; }
        return frc;
    }
    const int rc = dstream_windowless_step(s, c, method, comp_size, uncomp_size, hash, in, in_size, consumed);
    if (rc) return rc;
    return dstream_hand_out(s, method, out, out_cap, produced, done);
}

int zpk_cstream_create(zpk_codec* c, zpk_cstream** out)
{
    if (!c || !out) return ZPK_E_INVALID;
    zpk_cstream* s = new (std::nothrow) zpk_cstream();                                // (no member has an initialiser: all zero, the buffers empty)
    if (!s) return ZPK_E_NOMEM;
    s->c = c; s->device = c->device; *out = s;
    return ZPK_OK;
}

static void cstream_release(zpk_cstream* s)
{
    if (!s || !(s->d_in || s->d_out || s->d_slots || s->d_aux)) return;
    if (hipSetDevice(s->device) != hipSuccess) return;
    s->d_in.release(); s->d_out.release(); s->d_slots.release(); s->d_aux.release();
}

void zpk_cstream_bind(zpk_cstream* s, zpk_codec* c)
{
    if (!s || !c) return;
    if (s->device != c->device) cstream_release(s);
    s->c = c; s->device = c->device;
}
void zpk_cstream_reset(zpk_cstream* s)
{
    if (!s) return;
    s->in_len = 0; s->out_len = 0; s->out_pos = 0; s->total_in = 0; s->total_out = 0; s->configured = 0; s->steps = 0; s->framed = 0;
    if (s->d_in.cap + s->d_out.cap + s->d_slots.cap > (64ull << 20)) cstream_release(s);
}
void zpk_cstream_destroy(zpk_cstream* s) { if (s) { cstream_release(s); delete s; } }

// method and level of the entry being written: from here on zpk_cstream_update compresses as the plaintext arrives
int zpk_cstream_configure(zpk_cstream* s, uint32_t method, int32_t level)
{
    if (!s || !s->c) return 21;
    if (method != ZPK_METHOD_NONE && method != ZPK_METHOD_ZSTD && method != ZPK_METHOD_LZ4) return 19;
    if (s->total_in != 0) return 21;
    s->method = method; s->level = level; s->configured = 1;
    return 0;
}

#define ZPK_CS_AUX_STATE 0u
#define ZPK_CS_AUX_DESC  256u
#define ZPK_CS_AUX_RES   (ZPK_CS_AUX_DESC + 16u * (u32)sizeof(zpk_encode_desc))
#define ZPK_CS_AUX_OFFS  (ZPK_CS_AUX_RES + 16u * (u32)sizeof(zpk_encode_result))
#define ZPK_CS_AUX_BYTES (ZPK_CS_AUX_OFFS + 32u * 8u)

// a few bytes of the host's behind what is waiting to be handed out (the header / the end of a frame that goes out in pieces)
static int cstream_append(zpk_cstream* s, const u8* bytes, u32 n)
{
    zpk_codec* c = s->c;
    if (dgrow_keep(c, s->d_out, s->out_len + n + 64, s->out_len) != ZPK_OK) return 10;
    if (hipMemcpyAsync(s->d_out + s->out_len, bytes, n, hipMemcpyHostToDevice, c->stream) != hipSuccess) return 24;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return 24;              // (the bytes are the caller's stack)
    s->out_len += n; s->total_out += n;
    return 0;
}

// compress the first `npieces` pieces of the buffered plaintext (`last_len` = length of the last one; the others ZPK_ENC_PIECE) into
// frames appended to d_out; `hash_blocks`: whole 1 KiB blocks of those bytes to feed to the running XXH3
static int cstream_step(zpk_cstream* s, u32 npieces, u64 last_len, u64 hash_blocks, u64 src_off = 0, bool sequence = true)
{
    zpk_codec* c = s->c;
    u8* const plain = s->d_in + ZPK_CS_CARRY + src_off;
    zpk_cs_state* const st = (zpk_cs_state*)(s->d_aux + ZPK_CS_AUX_STATE);
    if (hash_blocks) hipLaunchKernelGGL(k_xxh3s_blocks, dim3(1), dim3(64), 0, c->stream, st, (const u8*)plain, hash_blocks);
    const u64 bytes = (u64)(npieces - 1) * ZPK_ENC_PIECE + last_len;
    if (s->method == ZPK_METHOD_NONE) {
        if (dgrow_keep(c, s->d_out, s->out_len + bytes + 64, s->out_len) != ZPK_OK) return 10;
        if (bytes && hipMemcpyAsync(s->d_out + s->out_len, plain, bytes, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) return 24;
        s->out_len += bytes; s->total_out += bytes; s->steps++;
        return hipStreamSynchronize(c->stream) == hipSuccess ? 0 : 24;
    }
    const u64 bound = zpk_codec_compress_bound(s->method, ZPK_ENC_PIECE), slot = (bound + 255) & ~255ull;
    if (dgrow_keep(c, s->d_slots, slot * ZPK_CS_PIECES + 64, 0) != ZPK_OK) return 10;
    if (sequence && !s->framed) {
        // an entry that goes out in pieces is ONE frame (round 5; what the reference's streaming writer keeps open across calls,
        // lib/zpack_write.c:477-574): its header now — no content size, it is not known yet —, the pieces as runs of blocks, the end of
        // the frame in zpk_cstream_finish
        const EncEnvelope E = enc_envelope(s->method, ZPK_ENC_SIZE_UNKNOWN);
        const int hrc = cstream_append(s, E.hdr, E.hl);
        if (hrc) return hrc;
        s->framed = 1;
    }
    // (not enc_emit_entry's slots: every piece of a step, a short last one too, has a full piece's bound: the array is laid out once)
    zpk_encode_desc hd[ZPK_CS_PIECES]; memset(hd, 0, sizeof(hd));
    for (u32 k = 0; k < npieces; k++) {
        hd[k].src_offset = (u64)k * ZPK_ENC_PIECE; hd[k].size = k + 1 == npieces ? last_len : (u64)ZPK_ENC_PIECE;
        hd[k].dst_offset = (u64)k * slot; hd[k].dst_capacity = bound; hd[k].method = s->method | (sequence ? ZPK_EF_PIECE : 0u); hd[k].level = s->level;   // (an entry of ONE frame is written exactly as the batch writer writes it)
    }
    zpk_encode_desc* const dd = (zpk_encode_desc*)(s->d_aux + ZPK_CS_AUX_DESC);
    zpk_encode_result* const dr = (zpk_encode_result*)(s->d_aux + ZPK_CS_AUX_RES);
    u64* const doff = (u64*)(s->d_aux + ZPK_CS_AUX_OFFS);
    if (hipMemcpyAsync(dd, hd, npieces * sizeof(zpk_encode_desc), hipMemcpyHostToDevice, c->stream) != hipSuccess) return 24;
    if (zpk_codec_encode_batch_device(c, plain, bytes + 16, dd, npieces, s->d_slots, slot * ZPK_CS_PIECES, dr, c->stream) != ZPK_OK) return 24;
    // the frames back to back behind what is still waiting to be handed out
    if (dgrow_keep(c, s->d_out, s->out_len + bound * npieces + 64, s->out_len) != ZPK_OK) return 10;
    if (zpk_codec_pack_batch_device(c, s->d_slots, dd, dr, npieces, s->d_out + s->out_len, bound * npieces, doff, bound, c->stream) != ZPK_OK) return 24;
    zpk_encode_result hr[ZPK_CS_PIECES]; u64 hoff[ZPK_CS_PIECES + 1];
    hipError_t e = hipMemcpyAsync(hr, dr, npieces * sizeof(zpk_encode_result), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(hoff, doff, (npieces + 1) * sizeof(u64), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return 24;
    for (u32 k = 0; k < npieces; k++) if (hr[k].status) return hr[k].status;
    s->out_len += hoff[npieces]; s->total_out += hoff[npieces]; s->steps++;
    return 0;
}

// the plaintext goes to the DEVICE (the host holds nothing but the caller's chunk); complete pieces are compressed as they come
int zpk_cstream_update(zpk_cstream* s, const uint8_t* in, size_t in_size)
{
    if (!s || !s->c) return 21;
    if (!in_size) return 0;
    zpk_codec* c = s->c;
    CodecLock lk(c);
    if (hipSetDevice(c->device) != hipSuccess) return 24;
    if (!s->configured) { s->method = ZPK_METHOD_NONE; s->level = 0; }        // (a caller that never configures: everything is compressed by zpk_cstream_finish)
    if (dgrow_keep(c, s->d_aux, ZPK_CS_AUX_BYTES, 0) != ZPK_OK) return 10;
    if (s->total_in == 0) {
        hipLaunchKernelGGL(k_xxh3s_init, dim3(1), dim3(64), 0, c->stream, (zpk_cs_state*)(s->d_aux + ZPK_CS_AUX_STATE));
        if (dgrow_keep(c, s->d_in, ZPK_CS_CARRY + 64, 0) != ZPK_OK) return 10;
        if (hipMemsetAsync(s->d_in, 0, ZPK_CS_CARRY, c->stream) != hipSuccess) return 24;
    }
    while (in_size) {
        // take what fits under the next step's threshold + 1 byte: a piece is compressed only when a byte FOLLOWS it, so that none of its
        // 1 KiB blocks is the input's last (XXH3 treats that one differently).  First step after 512 KiB (first output early), then
        // eight pieces at a time.
        const u64 thr = !s->configured ? ~0ull >> 2 : (s->steps == 0 ? (u64)ZPK_ENC_PIECE : (u64)ZPK_ENC_PIECE * ZPK_CS_PIECES);
        const u64 room = thr + 1 - s->in_len;                               // (in_len <= thr here: a step leaves at most one piece behind)
        const u64 take = in_size < room ? in_size : room;
        if (dgrow_keep(c, s->d_in, ZPK_CS_CARRY + s->in_len + take + 64, ZPK_CS_CARRY + s->in_len) != ZPK_OK) return 10;
        if (hipMemcpyAsync(s->d_in + ZPK_CS_CARRY + s->in_len, in, take, hipMemcpyHostToDevice, c->stream) != hipSuccess) return 24;
        s->in_len += take; s->total_in += take; in += take; in_size -= take;
        if (s->in_len > thr) {
            const u32 np = (u32)((s->in_len - 1) / ZPK_ENC_PIECE);                       // >= 1 whole pieces with a byte behind them
            const u64 bytes = (u64)np * ZPK_ENC_PIECE;
            const int rc = cstream_step(s, np, ZPK_ENC_PIECE, bytes >> 10);
            if (rc) return rc;
            // what is left moves to the front, behind the 64 bytes that precede it
            const u64 rest = s->in_len - bytes;
            if (hipMemcpyAsync(s->d_in, s->d_in + bytes, ZPK_CS_CARRY, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) return 24;   // (bytes >= 512 KiB: no overlap)
            if (rest && hipMemcpyAsync(s->d_in + ZPK_CS_CARRY, s->d_in + ZPK_CS_CARRY + bytes, rest, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) return 24;
            s->in_len = rest;
        }
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess) return 24;          // the caller may reuse its window at once
    return 0;
}

// the rest of the plaintext (and, for an entry that never reached a step, all of it); the XXH3 of the whole entry
int zpk_cstream_finish(zpk_cstream* s, uint32_t method, int32_t level, uint64_t* comp_size, uint64_t* uncomp_size, uint64_t* hash)
{
    if (!s || !s->c) return 21;
    zpk_codec* c = s->c;
    CodecLock lk(c);
    if (hipSetDevice(c->device) != hipSuccess) return 24;
    if (!s->configured || s->total_in == 0) { s->method = method; s->level = level; }
    if (dgrow_keep(c, s->d_aux, ZPK_CS_AUX_BYTES, 0) != ZPK_OK) return 10;
    if (dgrow_keep(c, s->d_in, ZPK_CS_CARRY + s->in_len + 64, s->total_in ? ZPK_CS_CARRY + s->in_len : 0) != ZPK_OK) return 10;   // (an empty entry that never saw an update: still a buffer to point at, nothing to keep)
    zpk_cs_state* const st = (zpk_cs_state*)(s->d_aux + ZPK_CS_AUX_STATE);
    if (s->total_in == 0) hipLaunchKernelGGL(k_xxh3s_init, dim3(1), dim3(64), 0, c->stream, st);
    hipLaunchKernelGGL(k_xxh3s_finish, dim3(1), dim3(64), 0, c->stream, st, (const u8*)(s->d_in + ZPK_CS_CARRY), s->in_len, s->total_in);
    // the remaining pieces (an entry that never stepped may hold more than eight: unconfigured callers); an empty entry is one empty frame
    u64 left = s->in_len, at = 0;
    bool any = s->steps == 0;
    const bool sequence = s->steps > 0 || left > ZPK_ENC_PIECE;
    while (left || any) {
        any = false;
        u32 np = (u32)((left + ZPK_ENC_PIECE - 1) / ZPK_ENC_PIECE); if (np == 0) np = 1; if (np > ZPK_CS_PIECES) np = ZPK_CS_PIECES;
        const u64 bytes = (u64)np * ZPK_ENC_PIECE < left ? (u64)np * ZPK_ENC_PIECE : left;
        const u64 last_len = bytes - (u64)(np - 1) * ZPK_ENC_PIECE;
        const int rc = cstream_step(s, np, last_len, 0, at, sequence);
        if (rc) return rc;
        left -= bytes; at += bytes;
    }
    if (s->framed) {                                                         // the end of the frame: LZ4 EndMark / an empty last Zstandard block
        const EncEnvelope E = enc_envelope(s->method, ZPK_ENC_SIZE_UNKNOWN);
        const int trc = cstream_append(s, E.trl, E.tl);
        if (trc) return trc;
    }
    zpk_cs_state hs;
    if (hipMemcpy(&hs, st, sizeof(hs), hipMemcpyDeviceToHost) != hipSuccess) return 24;
    s->in_len = 0;
    if (comp_size) *comp_size = s->total_out;
    if (uncomp_size) *uncomp_size = s->total_in;
    if (hash) *hash = hs.hash;
    return 0;
}

size_t zpk_cstream_drain(zpk_cstream* s, uint8_t* out, size_t out_cap)
{
    if (!s || !s->c) return 0;
    u64 left = s->out_len - s->out_pos;
    u64 give = out_cap < left ? out_cap : left;
    if (give) {
        CodecLock lk(s->c);
        if (hipSetDevice(s->c->device) != hipSuccess) return 0;
        if (hipMemcpy(out, s->d_out + s->out_pos, give, hipMemcpyDeviceToHost) != hipSuccess) return 0;
    }
    s->out_pos += give;
    if (s->out_pos == s->out_len) { s->out_pos = 0; s->out_len = 0; }      // everything handed out: the next frames start at the front
    return (size_t)give;
}

}  // extern "C"
