// zpk_dsink.inc — a batch compressed INTO A BOUNDED SINK IN THE CALLER'S DEVICE MEMORY (zpk_codec_encode_batch_dsink) and the small
// host-built blocks that go there (zpk_codec_store_device): what libzpack_amd.so writes an archive image in device memory with
// (zpack_amd.h: zpack_amd_init_writer_device).  The rules are dsink_plan.h's, the two kernels sink_commit.h's; they are compiled in a file
// of their own (sink_commit.hip), as k_span_copy is.
namespace zpk {
void sink_commit_launch(const u8* d_slots, const u64* d_slot_off, const zpk_encode_result* d_res, const u64* d_offsets, const u64* d_span_first,
                        u32 n, u64 room, u64* d_rec, u8* d_sink, u32 grid, hipEvent_t ev0, hipEvent_t ev1, hipStream_t st);
}

// workgroups of four waves the chip holds at once at k_sink_place's occupancy of 8 waves per SIMD
static u32 sink_resident_groups(zpk_codec* c)
{
    if (!c->sink_groups) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || cus <= 0) { (void)hipGetLastError(); cus = 256; }
        c->sink_groups = (u32)cus * 8u;
    }
    return c->sink_groups;
}

// One sub-batch: desc[0, m) staged, encoded into slots of the codec's, scanned, cut against `room` and committed to d_sink; results[0, m)
// and the cut come home in one copy.  Returns when the sink holds the bytes.
static int dsink_sub(zpk_codec* c, const uint8_t* const* src_ptrs, bool dsrc, const zpk_encode_desc* desc, u64 m, u8* d_sink, u64 room,
                     zpk_encode_result* results, SinkCut* cut)
{
    std::vector<zpk_encode_desc> hd;
    std::vector<u64> slot_off;
    std::vector<u8> home;
    const u64 res_bytes = m * sizeof(zpk_encode_result), home_bytes = res_bytes + 2 * sizeof(u64);
    try { hd.assign(desc, desc + m); slot_off.resize(m); home.resize(home_bytes); } catch (...) { return ZPK_E_NOMEM; }
    u64 in_total = 0, out_total = 0, items_bound = 0;
    for (u64 i = 0; i < m; i++) {
        const u64 si = sink_src_slot(desc[i].size), so = sink_slot(desc[i].dst_capacity);
        if (si > (1ull << 62) - in_total || so > (1ull << 62) - out_total) { snprintf(c->err, sizeof(c->err), "entry %llu: no staging of that size", (unsigned long long)i); return ZPK_E_NOMEM; }
        hd[i].src_offset = in_total; hd[i].dst_offset = slot_off[i] = out_total;
        in_total += si; out_total += so;
        items_bound = sink_items_bound(items_bound, desc[i].dst_capacity);
    }
    if (items_bound > 0xFFFFFFF0ull) return ZPK_E_INVALID;                             // (k_sink_place dequeues with 32-bit item numbers: 64 TiB of slots)
    // the tables of the commit, one block: results | record | offsets | slot offsets
    const u64 o_rec = res_bytes, o_off = o_rec + SINK_REC_WORDS * sizeof(u64), o_slot = o_off + (m + 1) * sizeof(u64);
    const u64 nblocks = (m + PK_BLOCK - 1) / PK_BLOCK;
    int rc;
    if ((rc = grow(c, c->d_src, in_total + 64)) || (rc = grow(c, c->d_sink_slots, out_total + 64)) ||
        (rc = grow(c, c->d_sink_tab, o_slot + m * sizeof(u64)))) return rc;
    hipStream_t st = c->stream;
    hipError_t e = hipSuccess;
    if (dsrc) {                                                                       // DEVICE sources: ONE launch of k_span_copy, as zpk_codec_encode_batch_dsrc
        std::vector<zpk_span_copy> sp;
        try { sp.reserve(m); } catch (...) { return ZPK_E_NOMEM; }
        for (u64 i = 0; i < m; i++) if (desc[i].size) sp.push_back(zpk_span_copy{ (u64)src_ptrs[i], (u64)(c->d_src + hd[i].src_offset), desc[i].size });
        if ((rc = span_copy_enqueue(c, sp.data(), sp.size(), st))) return rc;
    }
    else if (m == 1) { if (desc[0].size) e = hipMemcpyAsync(c->d_src, src_ptrs[0], desc[0].size, hipMemcpyHostToDevice, st); }
    else {
        const int grc = h2d_gather(c, c->d_src, in_total, m, src_ptrs, [&](u64 i) { return (u64)hd[i].src_offset; }, [&](u64 i) { return (u64)desc[i].size; }, e, st);
        if (grc) return grc;
    }
    u8* const tab = c->d_sink_tab;
    zpk_encode_result* const d_res = (zpk_encode_result*)tab;
    u64* const d_rec = (u64*)(tab + o_rec); u64* const d_off = (u64*)(tab + o_off); u64* const d_slot = (u64*)(tab + o_slot);
    if (e == hipSuccess) e = hipMemcpyAsync(d_slot, slot_off.data(), m * sizeof(u64), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) { snprintf(c->err, sizeof(c->err), "H2D: %s", hipGetErrorString(e)); return ZPK_E_LAUNCH; }
    // the frames, into the slots: large entries in pieces with their frame assembled on the device, every other entry by the one-wave launch
    if ((rc = zpk_codec_encode_big_device(c, c->d_src, in_total, hd.data(), m, c->d_sink_slots, out_total, d_res, st))) return rc;
    // where they go: the sizes-only scan, and the same scan over the entries' spans (pack_launch's layout of c->d_pack, which it has grown)
    if ((rc = pack_launch(c, nullptr, nullptr, d_res, m, nullptr, 0, d_off, 0, st))) return rc;
    u64* const span_blocks = (u64*)c->d_pack + nblocks;
    u64* const span_first = span_blocks + nblocks;
    hipLaunchKernelGGL(k_pack_block_sums<1>, dim3((u32)nblocks), dim3(256), 0, st, (const zpk_encode_result*)d_res, m, span_blocks);
    hipLaunchKernelGGL(k_pack_scan_blocks, dim3(1), dim3(256), 0, st, span_blocks, nblocks, span_first + m);
    hipLaunchKernelGGL(k_pack_offsets<1>, dim3((u32)nblocks), dim3(256), 0, st, (const zpk_encode_result*)d_res, m, (const u64*)span_blocks, span_first);
    HIPCHK(c, hipGetLastError());
    // the commit
    const u32 grid = sink_grid(items_bound, sink_resident_groups(c));
    sink_commit_launch(c->d_sink_slots, d_slot, d_res, d_off, span_first, (u32)m, room, d_rec, d_sink, grid,
                       c->profiling ? c->kev[ZPK_K_PACK][0] : nullptr, c->profiling ? c->kev[ZPK_K_PACK][1] : nullptr, st);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(home.data(), tab, home_bytes, hipMemcpyDeviceToHost, st));          // [results | cut record], one copy
    HIPCHK(c, hipStreamSynchronize(st));
    memcpy(results, home.data(), res_bytes);
    u64 rec[2];
    memcpy(rec, home.data() + res_bytes, sizeof(rec));
    cut->placed = rec[0]; cut->bytes = rec[1];
    if (cut->placed > m || cut->bytes > room) { snprintf(c->err, sizeof(c->err), "sink commit: a cut of %llu entries, %llu bytes", (unsigned long long)rec[0], (unsigned long long)rec[1]); return ZPK_E_LAUNCH; }
    c->dsink_last[0]++; c->dsink_last[1] = grid;
    return ZPK_OK;
}

extern "C" {

// instance-free, the mirror of zpk_codec_fetch_device: [host_src, + bytes) to d_dst, when that is `bytes` bytes of one allocation in device memory
int zpk_codec_store_device(void* d_dst, const void* host_src, uint64_t bytes)
{
    if (zpk_codec_device_count() <= 0) return ZPK_E_NO_DEVICE;
    if (bytes == 0) return ZPK_OK;
    hipPointerAttribute_t at;
    if (!d_dst || hipPointerGetAttributes(&at, d_dst) != hipSuccess) { (void)hipGetLastError(); return ZPK_E_INVALID; }
    if (at.type != hipMemoryTypeDevice) return ZPK_E_INVALID;
    int was = -1;
    if (hipGetDevice(&was) != hipSuccess) { (void)hipGetLastError(); was = -1; }
    if (was != at.device && hipSetDevice(at.device) != hipSuccess) { (void)hipGetLastError(); return ZPK_E_LAUNCH; }
    hipDeviceptr_t base = nullptr; size_t size = 0;
    int rc = ZPK_OK;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)d_dst) != hipSuccess) { (void)hipGetLastError(); rc = ZPK_E_INVALID; }
    else if (!span_copy_in_range((u64)d_dst, bytes, (u64)base, size)) rc = ZPK_E_INVALID;
    else if (host_src && hipMemcpy(d_dst, host_src, bytes, hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); rc = ZPK_E_LAUNCH; }
    if (was >= 0 && was != at.device) (void)hipSetDevice(was);
    return rc;
}

int zpk_codec_encode_batch_dsink(zpk_codec* c, const uint8_t* const* src_ptrs, int src_on_device, const zpk_encode_desc* desc, uint64_t n,
                                 uint8_t* d_sink, uint64_t sink_room_bytes, zpk_encode_result* results, uint64_t* placed, uint64_t* bytes)
{
    if (!c || !placed || !bytes || (n && (!desc || !results || !src_ptrs))) return ZPK_E_INVALID;
    *placed = 0; *bytes = 0;
    CodecLock lk(c);
    c->dsink_last[0] = c->dsink_last[1] = 0;
    if (n == 0) return ZPK_OK;
    HIPCHK(c, hipSetDevice(c->device));
    // the pointer check: before anything is enqueued.  The sink and device sources lie inside one allocation each on this device; a host
    // source is not device memory (a device pointer in a host array would be read by the host)
    span_check_begin(c);
    if (!span_ptr_ok(c, d_sink, sink_room_bytes)) { snprintf(c->err, sizeof(c->err), "the sink is not %llu bytes of one allocation on device %d", (unsigned long long)sink_room_bytes, c->device); return ZPK_E_INVALID; }
    for (u64 i = 0; i < n; i++) {
        const bool ok = src_on_device ? span_ptr_ok(c, src_ptrs[i], desc[i].size) : (desc[i].size == 0 || (src_ptrs[i] && zpk_codec_pointer_device(src_ptrs[i]) < 0));
        if (!ok) { snprintf(c->err, sizeof(c->err), "source %llu is not %llu bytes of %s memory", (unsigned long long)i, (unsigned long long)desc[i].size, src_on_device ? "this device's" : "host"); return ZPK_E_INVALID; }
    }
    const u64 chunk = dimage_chunk(c->dimage_chunk);
    SinkChain ch = { 0, 0, true };
    for (u64 first = 0; first < n && ch.open; ) {
        const DimageCut sub = dimage_cut(first, n, chunk, [&](u64 i) { return sink_slot(desc[i].dst_capacity); });
        SinkCut cut = { 0, 0 };
        const int rc = dsink_sub(c, src_ptrs + first, src_on_device != 0, desc + first, sub.count, d_sink + ch.bytes, sink_room(sink_room_bytes, ch.bytes), results + first, &cut);
        if (rc) { *placed = ch.placed; *bytes = ch.bytes; return rc; }
        sink_chain(ch, sub.count, cut);
        first += sub.count;
    }
    *placed = ch.placed; *bytes = ch.bytes;
    return ZPK_OK;
}

// waits for what the codec's own stream holds (zpk_codec_copy_spans_device enqueues there and returns)
int zpk_codec_stream_sync(zpk_codec* c)
{
    if (!c) return ZPK_E_INVALID;
    CodecLock lk(c);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ZPK_OK;
}

int zpk_codec_dsink_stats(zpk_codec* c, uint32_t out[4])
{
    if (!c || !out) return ZPK_E_INVALID;
    CodecLock lk(c);
    out[0] = c->dsink_last[0]; out[1] = c->dsink_last[1]; out[2] = out[3] = 0;
    return ZPK_OK;
}

}  // extern "C"
