// zpk_dsink.inc — a batch compressed INTO A BOUNDED SINK IN THE CALLER'S DEVICE MEMORY (zpk_codec_encode_batch_dsink): what libzpack_amd.so
// writes an archive image in device memory with (zpack_amd.h: zpack_amd_init_writer_device).  The rules are dsink_plan.h's, the two kernels
// sink_commit.h's; they are compiled in a file of their own (sink_commit.hip), as k_span_copy is.  What it shares with the other
// device-memory paths is in zpk_codec.hip: the pointer rule (PtrRule over device_range_of), the staging of a sub-batch's sources
// (stage_sources) and the checked copy behind zpk_codec_store_device, with which the small host-built blocks go to the sink.
namespace zpk {
void sink_commit_launch(const u8* d_slots, const u64* d_slot_off, const zpk_encode_result* d_res, const u64* d_offsets, const u64* d_span_first,
                        u32 n, u64 room, u64* d_rec, u8* d_sink, u32 grid, hipEvent_t ev0, hipEvent_t ev1, hipStream_t st);
}

// workgroups of four waves the chip holds at once at k_sink_place's occupancy of 8 waves per SIMD
static u32 sink_resident_groups(zpk_codec* c)
{
    if (!c->sink.groups) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || cus <= 0) { (void)hipGetLastError(); cus = 256; }
        c->sink.groups = (u32)cus * 8u;
    }
    return c->sink.groups;
}

// One sub-batch: desc[0, m) staged, encoded into slots of the codec's, scanned, cut against `room` and committed to d_sink; results[0, m)
// and the cut come home in one copy.  Returns when the sink holds the bytes.
static int dsink_sub(zpk_codec* c, const uint8_t* const* src_ptrs, bool dsrc, const zpk_encode_desc* desc, u64 m, u8* d_sink, u64 room,
                     zpk_encode_result* results, SinkCut* cut, const Planes& pl)
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
    if ((rc = grow(c, c->d_src, in_total + 64)) || (rc = grow(c, c->sink.d_slots, out_total + 64)) ||
        (rc = grow(c, c->sink.d_tab, o_slot + m * sizeof(u64)))) return rc;
    hipStream_t st = c->stream;
    hipError_t e = hipSuccess;
    // the sources, as zpk_codec_encode_batch_host / _dsrc stage them (zpk_codec.hip, stage_sources)
    if ((rc = stage_sources(c, src_ptrs, dsrc, m, [&](u64 i) { return (u64)hd[i].src_offset; }, [&](u64 i) { return (u64)desc[i].size; }, in_total, st, e, pl))) return rc;
    u8* const tab = c->sink.d_tab;
    zpk_encode_result* const d_res = (zpk_encode_result*)tab;
    u64* const d_rec = (u64*)(tab + o_rec); u64* const d_off = (u64*)(tab + o_off); u64* const d_slot = (u64*)(tab + o_slot);
    if (e == hipSuccess) e = hipMemcpyAsync(d_slot, slot_off.data(), m * sizeof(u64), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) { snprintf(c->err, sizeof(c->err), "H2D: %s", hipGetErrorString(e)); return ZPK_E_LAUNCH; }
    // the frames, into the slots: large entries in pieces with their frame assembled on the device, every other entry by the one-wave launch
    if ((rc = zpk_codec_encode_big_device(c, c->d_src, in_total, hd.data(), m, c->sink.d_slots, out_total, d_res, st))) return rc;
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
    sink_commit_launch(c->sink.d_slots, d_slot, d_res, d_off, span_first, (u32)m, room, d_rec, d_sink, grid,
                       c->profiling ? c->kev[ZPK_K_PACK][0] : nullptr, c->profiling ? c->kev[ZPK_K_PACK][1] : nullptr, st);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(home.data(), tab, home_bytes, hipMemcpyDeviceToHost, st));          // [results | cut record], one copy
    HIPCHK(c, hipStreamSynchronize(st));
    memcpy(results, home.data(), res_bytes);
    u64 rec[2];
    memcpy(rec, home.data() + res_bytes, sizeof(rec));
    cut->placed = rec[0]; cut->bytes = rec[1];
    if (cut->placed > m || cut->bytes > room) { snprintf(c->err, sizeof(c->err), "sink commit: a cut of %llu entries, %llu bytes", (unsigned long long)rec[0], (unsigned long long)rec[1]); return ZPK_E_LAUNCH; }
    c->last.dsink[0]++; c->last.dsink[1] = grid;
    return ZPK_OK;
}

extern "C" {

// (elem: the element sizes of DEVICE sources, plane_copy_plan.h — NULL: every entry is plain bytes; host sources take no other.
// d_base: their bases, delta_copy_plan.h — NULL, or NULL for an entry: no base; host sources take none)
int zpk_codec_encode_batch_dsink_delta(zpk_codec* c, const uint8_t* const* src_ptrs, int src_on_device, const zpk_encode_desc* desc, uint64_t n,
                                       uint8_t* d_sink, uint64_t sink_room_bytes, zpk_encode_result* results, uint64_t* placed, uint64_t* bytes,
                                       const uint8_t* elem, const uint8_t* const* d_base)
{
    if (!c || !placed || !bytes || (n && (!desc || !results || !src_ptrs))) return ZPK_E_INVALID;
    *placed = 0; *bytes = 0;
    CodecLock lk(c);
    c->last.dsink[0] = c->last.dsink[1] = 0;
    c->last.no_planes();
    if (n == 0) return ZPK_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (planes_check(c, elem, n)) return ZPK_E_INVALID;
    for (u64 i = 0; elem && !src_on_device && i < n; i++) if (elem[i] != 1) { snprintf(c->err, sizeof(c->err), "source %llu: an element size of %u for host memory", (unsigned long long)i, (unsigned)elem[i]); return ZPK_E_INVALID; }
    for (u64 i = 0; d_base && !src_on_device && i < n; i++) if (d_base[i]) { snprintf(c->err, sizeof(c->err), "source %llu: a base for host memory", (unsigned long long)i); return ZPK_E_INVALID; }
    const Planes pl = { src_on_device ? elem : nullptr, src_on_device ? d_base : nullptr };
    // the pointer rule (zpk_codec.hip, PtrRule): before anything is enqueued.  The sink and device sources lie inside one allocation each on
    // this device; a host source with bytes is not device memory (the host would read through such a pointer)
    PtrRule rule(c);
    if (rule.batch("sink", 1, [&](u64) { return d_sink; }, [&](u64) { return (u64)sink_room_bytes; }) ||
        (src_on_device && rule.batch("source", n, [&](u64 i) { return src_ptrs[i]; }, [&](u64 i) { return (u64)desc[i].size; }))) return ZPK_E_INVALID;
    if (bases_check(c, rule, pl, n, [&](u64 i) { return (u64)desc[i].size; }, nullptr)) return ZPK_E_INVALID;
    for (u64 i = 0; i < n && !src_on_device; i++)
        if (desc[i].size && (!src_ptrs[i] || zpk_codec_pointer_device(src_ptrs[i]) >= 0)) {
            snprintf(c->err, sizeof(c->err), "source %llu is not %llu bytes of host memory (the codec of device %d reads it on the host)", (unsigned long long)i, (unsigned long long)desc[i].size, c->device);
            return ZPK_E_INVALID;
        }
    const u64 chunk = dimage_chunk(c->opt.dimage_chunk);
    SinkChain ch = { 0, 0, true };
    for (u64 first = 0; first < n && ch.open; ) {
        const DimageCut sub = dimage_cut(first, n, chunk, [&](u64 i) { return sink_slot(desc[i].dst_capacity); });
        SinkCut cut = { 0, 0 };
        const int rc = dsink_sub(c, src_ptrs + first, src_on_device != 0, desc + first, sub.count, d_sink + ch.bytes, sink_room(sink_room_bytes, ch.bytes), results + first, &cut, pl.from(first));
        if (rc) { *placed = ch.placed; *bytes = ch.bytes; return rc; }
        sink_chain(ch, sub.count, cut);
        first += sub.count;
    }
    *placed = ch.placed; *bytes = ch.bytes;
    return ZPK_OK;
}

int zpk_codec_encode_batch_dsink_planes(zpk_codec* c, const uint8_t* const* src_ptrs, int src_on_device, const zpk_encode_desc* desc, uint64_t n,
                                        uint8_t* d_sink, uint64_t sink_room_bytes, zpk_encode_result* results, uint64_t* placed, uint64_t* bytes,
                                        const uint8_t* elem)
{
    return zpk_codec_encode_batch_dsink_delta(c, src_ptrs, src_on_device, desc, n, d_sink, sink_room_bytes, results, placed, bytes, elem, nullptr);
}

int zpk_codec_encode_batch_dsink(zpk_codec* c, const uint8_t* const* src_ptrs, int src_on_device, const zpk_encode_desc* desc, uint64_t n,
                                 uint8_t* d_sink, uint64_t sink_room_bytes, zpk_encode_result* results, uint64_t* placed, uint64_t* bytes)
{
    return zpk_codec_encode_batch_dsink_planes(c, src_ptrs, src_on_device, desc, n, d_sink, sink_room_bytes, results, placed, bytes, nullptr);
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
    out[0] = c->last.dsink[0]; out[1] = c->last.dsink[1]; out[2] = out[3] = 0;
    return ZPK_OK;
}

}  // extern "C"
