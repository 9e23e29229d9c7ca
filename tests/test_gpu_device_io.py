"""GPU: the plaintext in DEVICE memory through the library API (include/zpack_amd.h: zpack_amd_read_files_device, _packed,
zpack_amd_write_files_device), the codec calls behind it and the kernel that moves the bytes (k_span_copy, zpack_amd/csrc/row_copy.hip).

The reference of every read is zpack_read_files of the same library with host buffers and the same arguments: same results, same bytes
in all of [buffer, buffer + max_size) — host and device buffers start out as 0xA5, so a byte the host path does not write must not be
written here either — the same last_return, and 64 canary bytes around every device destination intact.  The reference of every write is
zpack_write_files from host copies of the same bytes: the same archive byte for byte, and every entry decodes to its source through the
oracle.  Memory comes from torch."""
import ctypes as C
import os

import numpy as np
import pytest

import zpack_amd
from benchdata import datagen as dg
from tests import zpk
from tests._libs import Reader, Writer, File, FileEntry, CompressOptions, u8p, oracle, METHOD_NONE, METHOD_ZSTD, METHOD_LZ4
from tests.device_mem import torch, Z, _plain, _build, _layout, CANARY, GAP            # noqa: F401  (torch, Z: fixtures)

pytestmark = pytest.mark.gpu

PFE = C.POINTER(FileEntry)


# ------------------------------------------------------------------------------------------------ helpers

def _entry_ptrs(ents):
    return (PFE * max(len(ents), 1))(*[C.pointer(e) for e in ents])


def _read_host(Z, r, ents, caps):
    n = len(ents)
    bufs = [np.full(max(c, 1), CANARY, dtype=np.uint8) for c in caps]
    ptrs = (u8p * max(n, 1))(*[b.ctypes.data_as(u8p) for b in bufs])
    res = (C.c_int * max(n, 1))(*([-1] * max(n, 1)))
    rc = Z.lib.zpack_read_files(C.byref(r), _entry_ptrs(ents), n, ptrs, (C.c_size_t * max(n, 1))(*caps), res, None)
    return rc, list(res)[:n], [b[:c] for b, c in zip(bufs, caps)], int(r.last_return)


def _read_dev(Z, torch, r, ents, caps, mis=(0,), override=None, room=None):
    """-> rc, results, the whole device buffer (host copy), the destinations' offsets in it, last_return.  override: {i: address};
    room: the sizes the buffer is laid out for, where they are not the max_sizes handed to the call"""
    n = len(ents)
    offs, total = _layout(room or caps, mis)
    buf = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    addr = [buf.data_ptr() + o for o in offs]
    for i, a in (override or {}).items():
        addr[i] = a
    res = (C.c_int * max(n, 1))(*([-1] * max(n, 1)))
    rc = Z.lib.zpack_amd_read_files_device(C.byref(r), _entry_ptrs(ents), n, (C.c_void_p * max(n, 1))(*addr), (C.c_size_t * max(n, 1))(*caps), res, None)
    torch.cuda.synchronize()
    return rc, list(res)[:n], buf.cpu().numpy(), offs, int(r.last_return)


def _expected(total, offs, host_bufs):
    e = np.full(total, CANARY, dtype=np.uint8)
    for o, b in zip(offs, host_bufs):
        e[o:o + len(b)] = b
    return e


def _same_as_host(Z, torch, r, ents, caps, mis=(0,), bytes_of=(0, 15)):
    """one batch through both forms; the bytes of an entry are compared when the host's verdict is one of bytes_of (a decoder that gave
    up leaves what it had produced: the verdict is the contract there), the canaries and every other byte always"""
    hrc, hres, hbufs, hlast = _read_host(Z, r, ents, caps)
    drc, dres, dbuf, offs, dlast = _read_dev(Z, torch, r, ents, caps, mis)
    assert (drc, dres, dlast) == (hrc, hres, hlast)
    for i, (o, c) in enumerate(zip(offs, caps)):
        if hres[i] not in bytes_of:
            hbufs[i] = dbuf[o:o + c].copy()
    want = _expected(len(dbuf), offs, hbufs)
    if not np.array_equal(dbuf, want):
        bad = int(np.flatnonzero(dbuf != want)[0])
        k = max(i for i, o in enumerate(offs) if o - GAP <= bad) if bad >= offs[0] - GAP else -1
        raise AssertionError("byte %d of the device buffer differs (near destination %d at %d, %d bytes): %d, want %d"
                             % (bad, k, offs[k], caps[k], dbuf[bad], want[bad]))
    return hres


def _open(Z, arc):
    keep = (C.c_uint8 * len(arc)).from_buffer_copy(arc)
    r = Reader()
    assert Z.lib.zpack_init_reader_memory_shared(C.byref(r), C.cast(keep, u8p), len(arc)) == 0
    return r, keep


@pytest.fixture(scope="module")
def mixed():
    """~200 entries in the three methods: the sizes around 64 KiB, 0 and 1, a few up to 300 KiB, the rest small"""
    sizes = [0, 1, 65535, 65536, 65537] * 3 + [300 << 10, 200 * 1024 + 3, 131072 + 1, 100000]
    rng = np.random.default_rng(7)
    sizes += [int(x) for x in rng.integers(2, 6000, 201 - len(sizes))]
    methods = [(dg.NONE, 0), (dg.LZ4, 0), (dg.ZSTD, 3)]
    specs = []
    for i, n in enumerate(sizes):
        m, lv = methods[(i % 5 + i // 5) % 3]                                          # every edge size in every method
        specs.append((m, lv, _plain(i, n)))
    return _build(specs), [s[2] for s in specs]


# ------------------------------------------------------------------------------------------------ the kernel alone

def test_span_copy_kernel_lengths_and_alignments(torch):
    lens = [0, 1, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 16383, 16384, 16385, 32769]
    aligns = [(0, 0), (1, 0), (0, 1), (3, 13), (15, 15)]
    spans = [(n, sa, da) for (sa, da) in aligns for n in lens]
    rng = np.random.default_rng(3)
    spos, dpos, soffs, doffs = 16, GAP, [], []
    for n, sa, da in spans:
        spos = ((spos + 15) & ~15) + sa
        dpos = ((dpos + 15) & ~15) + da
        soffs.append(spos); doffs.append(dpos)
        spos += n + 1                                                                  # (sources one byte apart: a read past the end would show as a wrong byte nowhere, but stays inside the buffer)
        dpos += n + GAP
    src_h = rng.integers(0, 256, spos + 16, dtype=np.uint8)
    src = torch.from_numpy(src_h).to("cuda:0")
    dst = torch.full((dpos + GAP,), CANARY, dtype=torch.uint8, device="cuda:0")
    rows = np.array([[src.data_ptr() + so, dst.data_ptr() + do, n] for (n, _, _), so, do in zip(spans, soffs, doffs)], dtype=np.uint64)
    codec = zpack_amd.Codec(0)
    codec.copy_spans_device(rows)                                                     # ONE launch: 75 spans, 2 of them with two and 1 with three 16 KiB items
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    want = np.full(dpos + GAP, CANARY, dtype=np.uint8)
    for (n, _, _), so, do in zip(spans, soffs, doffs):
        want[do:do + n] = src_h[so:so + n]
    assert np.array_equal(got, want), int(np.flatnonzero(got != want)[0])
    assert np.array_equal(src.cpu().numpy(), src_h)
    # the pointer check of the call itself: a span that leaves its allocation, a host address — ZPK_E_INVALID (-2), nothing has run
    L = zpack_amd.lib()
    dst.fill_(CANARY); torch.cuda.synchronize()
    small = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    host = np.zeros(64, dtype=np.uint8)
    for bad in ([small.data_ptr(), dst.data_ptr() + GAP, 1 << 40], [host.ctypes.data, dst.data_ptr() + GAP, 64], [src.data_ptr(), 0, 16],
                [0, dst.data_ptr() + GAP, 16], [src.data_ptr(), host.ctypes.data, 64], [src.data_ptr(), small.data_ptr() + 100, 1 << 40]):
        both = np.array([[src.data_ptr(), dst.data_ptr() + GAP, 100], bad], dtype=np.uint64)
        assert L.zpk_codec_copy_spans_device(codec.h, both.ctypes.data, 2, None) == -2
    if torch.cuda.device_count() > 1:                                                  # memory of another device than the codec's, either end
        other = torch.full((4096,), CANARY, dtype=torch.uint8, device="cuda:1")
        torch.cuda.synchronize(1)
        for bad in ([other.data_ptr(), dst.data_ptr() + GAP, 64], [src.data_ptr(), other.data_ptr(), 64]):
            both = np.array([[src.data_ptr(), dst.data_ptr() + GAP, 100], bad], dtype=np.uint64)
            assert L.zpk_codec_copy_spans_device(codec.h, both.ctypes.data, 2, None) == -2
        torch.cuda.synchronize(1)
        assert bool((other == CANARY).all())
    torch.cuda.synchronize()
    assert bool((dst == CANARY).all()) and not host.any()
    # a span of no bytes passes wherever it points, NULL and host addresses included: the good row beside it is copied, and only that
    for nothing in ([0, 0, 0], [host.ctypes.data, host.ctypes.data + 8, 0]):
        both = np.array([nothing, [src.data_ptr(), dst.data_ptr() + GAP, 100]], dtype=np.uint64)
        assert L.zpk_codec_copy_spans_device(codec.h, both.ctypes.data, 2, None) == 0
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        assert np.array_equal(got[GAP:GAP + 100], src_h[:100]) and bool((got[:GAP] == CANARY).all()) and bool((got[GAP + 100:] == CANARY).all())
        dst.fill_(CANARY); torch.cuda.synchronize()
    assert not host.any()
    codec.close()


# ------------------------------------------------------------------------------------------------ reads

@pytest.mark.parametrize("arc", ["archive_none.zpk", "archive_zstd.zpk", "archive_lz4.zpk"])
@pytest.mark.parametrize("how", ["memory", "file"])
def test_golden_archives_read_like_zpack_read_files(Z, torch, golden_dir, arc, how):
    path = os.path.join(golden_dir, "ref_workdir", arc)
    if how == "file":
        r = Reader()
        assert Z.lib.zpack_init_reader(C.byref(r), path.encode()) == 0
    else:
        r, keep = _open(Z, open(path, "rb").read())
    try:
        ents = [r.file_entries[i] for i in range(r.file_count)]
        res = _same_as_host(Z, torch, r, ents, [350, 350], mis=(0, 5))
        assert res == [0, 0]
        drc, dres, dbuf, offs, _ = _read_dev(Z, torch, r, ents, [int(e.uncomp_size) for e in ents])
        for e, o, name in zip(ents, offs, ("file1.txt", "file2.txt")):
            assert dbuf[o:o + e.uncomp_size].tobytes() == open(os.path.join(golden_dir, "ref_workdir", name), "rb").read()
    finally:
        Z.lib.zpack_close_reader(C.byref(r))


def test_mixed_batch_shuffled_misaligned_and_packed(Z, torch, mixed):
    arc, plains = mixed
    r, keep = _open(Z, arc)
    try:
        n = int(r.file_count)
        order = list(np.random.default_rng(11).permutation(n))
        order.insert(50, order[3])                                                     # one entry twice, into two destinations
        if r.file_entries[order[-1]].uncomp_size == 0:                                 # (the packed form below wants bytes in its last entry)
            order.append(next(i for i in order if r.file_entries[i].uncomp_size > 1000))
        ents = [r.file_entries[i] for i in order]
        caps = [int(e.uncomp_size) + (7 if k % 4 == 1 else 0) for k, e in enumerate(ents)]      # some with room to spare
        res = _same_as_host(Z, torch, r, ents, caps, mis=(1, 7, 15))
        assert res == [0] * len(ents)
        drc, dres, dbuf, offs, _ = _read_dev(Z, torch, r, ents, caps, mis=(1, 7, 15))
        for i, o in zip(order, offs):
            assert dbuf[o:o + len(plains[i])].tobytes() == plains[i], i
        # ---- packed: offsets = running sum of uncomp_size rounded up to 256; the buffer one byte short for the last entry ----
        want_off, pos = [], 0
        for e in ents:
            want_off.append(pos)
            pos += (int(e.uncomp_size) + 255) & ~255
        size = want_off[-1] + int(ents[-1].uncomp_size) - 1
        buf = torch.full((size + GAP,), CANARY, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        offs_c = (C.c_uint64 * len(ents))()
        res_c = (C.c_int * len(ents))(*([-1] * len(ents)))
        rc = Z.lib.zpack_amd_read_files_device_packed(C.byref(r), _entry_ptrs(ents), len(ents), buf.data_ptr(), size, offs_c, res_c, None)
        torch.cuda.synchronize()
        assert rc == 0 and list(offs_c) == want_off
        assert list(res_c) == [0] * (len(ents) - 1) + [12]
        want = np.full(size + GAP, CANARY, dtype=np.uint8)
        for i, o in zip(order[:-1], want_off):
            want[o:o + len(plains[i])] = np.frombuffer(plains[i], dtype=np.uint8)
        got = buf.cpu().numpy()
        assert np.array_equal(got, want), int(np.flatnonzero(got != want)[0])
    finally:
        Z.lib.zpack_close_reader(C.byref(r))


def test_verdicts_in_one_batch_with_good_entries(Z, torch, mixed):
    arc, plains = mixed
    first = {}                                                                         # per method: an entry of a few KiB to damage
    ents0 = zpk.parse(arc)
    for i, e in enumerate(ents0):
        if e["uncomp_size"] > 3000 and e["comp_size"] > 200 and e["method"] not in first:
            first[e["method"]] = i
    assert sorted(first) == [0, 1, 2]
    damaged = bytearray(arc)
    for m, i in first.items():
        damaged[ents0[i]["offset"] + ents0[i]["comp_size"] // 2] ^= 0x40               # one flipped payload byte per method
    r, keep = _open(Z, bytes(damaged))
    try:
        good = [i for i in range(0, 40) if i not in first.values()]
        small, at_end, wrong_hash = [i for i in good[:20] if r.file_entries[i].uncomp_size > 1000][:3]
        ents, caps = [], []
        for i in good[:20] + list(first.values()):
            e = FileEntry.from_buffer_copy(r.file_entries[i])
            cap = int(e.uncomp_size)
            if i == small:
                cap -= 1
            if i == at_end:
                e.offset = len(arc) - e.comp_size                                      # offset + comp_size == file_size
            if i == wrong_hash:
                e.hash ^= 1
            ents.append(e); caps.append(cap)
        res = _same_as_host(Z, torch, r, ents, caps, mis=(0, 9))
        by = dict(zip(good[:20] + list(first.values()), res))
        assert by[small] == 12 and by[at_end] == 16 and by[wrong_hash] == 15
        assert by[first[0]] == 15                                                      # a stored entry with a flipped byte: the hash says so
        assert by[first[1]] != 0 and by[first[2]] != 0                                 # (whatever zpack_read_files says: _same_as_host compared)
        assert all(v == 0 for i, v in by.items() if i not in (small, at_end, wrong_hash) and i not in first.values())
    finally:
        Z.lib.zpack_close_reader(C.byref(r))


def test_large_entries_block_parallel_and_stored(Z, torch):
    n = (1 << 20) + 5
    specs = [(dg.LZ4, 0, _plain(0, n)), (dg.ZSTD, 3, _plain(3, n)), (dg.NONE, 0, _plain(1, 2 << 20)), (dg.LZ4, 0, _plain(6, 5000))]
    arc = _build(specs)
    r, keep = _open(Z, arc)
    try:
        ents = [r.file_entries[i] for i in range(r.file_count)]
        caps = [int(e.uncomp_size) for e in ents]
        res = _same_as_host(Z, torch, r, ents, caps, mis=(3, 0, 11))
        assert res == [0, 0, 0, 0]
        drc, dres, dbuf, offs, _ = _read_dev(Z, torch, r, ents, caps, mis=(3, 0, 11))
        for (m, lv, data), o in zip(specs, offs):
            assert dbuf[o:o + len(data)].tobytes() == data
    finally:
        Z.lib.zpack_close_reader(C.byref(r))
    # the codec call itself: the same entries take the same routes as in zpk_codec_decode_batch_host (block-parallel frames, a stored
    # entry in pieces), and say so in the same counters
    codec = zpack_amd.Codec(0)
    pe = zpk.parse(arc)
    desc = np.zeros(len(pe), dtype=zpack_amd.DECODE_DESC)
    for d, e in zip(desc, pe):
        d["src_offset"], d["comp_size"], d["uncomp_size"], d["expect_hash"] = e["offset"], e["comp_size"], e["uncomp_size"], e["hash"]
        d["dst_capacity"], d["method"] = e["uncomp_size"], e["method"]
    hres, houts = codec.decode_batch_host(arc, desc)
    hstats = codec.decode_stats()
    offs, total = _layout([int(x) for x in desc["dst_capacity"]], (3, 0, 11))
    buf = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda:0")
    dres = codec.decode_batch_host_dptr(arc, desc, [buf.data_ptr() + o for o in offs])
    dstats = codec.decode_stats()
    torch.cuda.synchronize()
    assert dres.tobytes() == hres.tobytes() and (hres["status"] == 0).all()
    print("routes: frame_parallel_entries %d, frames %d" % (hstats["frame_parallel_entries"], hstats["frame_parallel_frames"]))
    assert (dstats["frame_parallel_entries"], dstats["frame_parallel_frames"]) == (hstats["frame_parallel_entries"], hstats["frame_parallel_frames"])
    assert hstats["frame_parallel_entries"] >= 3                                       # the two frames block-parallel, the stored entry in pieces
    got = buf.cpu().numpy()
    assert np.array_equal(got, _expected(total, offs, houts))
    codec.close()


def test_sub_batch_that_takes_the_pipeline(torch):
    """3 x 4096 LZ4 entries with 3 x 64 MiB of output: the smallest sub-batch the host path decodes as a three-stage pipeline.  With
    device destinations the upload stays pipelined and a k_span_copy per piece stands where the download was."""
    n, size = 3 * 4096, 16384
    b = dg.Batch(n, size, size, method=dg.LZ4, level=0, seed=9)
    desc, _ = zpack_amd.decode_descs_from_batch(b)
    codec = zpack_amd.Codec(0)
    hres, houts = codec.decode_batch_host(b.archive, desc)
    hstats = codec.decode_stats()
    assert (hres["status"] == 0).all() and hstats["pipelined_sub_batches"] == 1 and hstats["span_copy_launches"] == 0
    at = GAP + 1                                                                       # every destination at an odd address
    buf = torch.full((at + n * size + GAP,), CANARY, dtype=torch.uint8, device="cuda:0")
    dres = codec.decode_batch_host_dptr(b.archive, desc, [buf.data_ptr() + at + i * size for i in range(n)])
    dstats = codec.decode_stats()
    torch.cuda.synchronize()
    assert dres.tobytes() == hres.tobytes()
    assert dstats["pipelined_sub_batches"] == 1 and dstats["span_copy_launches"] == 3  # one per piece
    got = buf.cpu().numpy()
    assert bool((got[:at] == CANARY).all()) and bool((got[at + n * size:] == CANARY).all())
    assert np.array_equal(got[at:at + n * size], np.concatenate(houts))
    assert got[at:at + size].tobytes() == b.plaintext(0).tobytes()
    codec.close()
    b.close()


def test_pointer_check_null_and_host_addresses(Z, torch, mixed):
    arc, plains = mixed
    r, keep = _open(Z, arc)
    try:
        idx = [i for i in range(r.file_count) if r.file_entries[i].uncomp_size > 100][:6]
        ents = [r.file_entries[i] for i in idx]
        caps = [int(e.uncomp_size) for e in ents]
        host = np.full(max(caps) + 64, CANARY, dtype=np.uint8)
        for override in ({2: None}, {4: host.ctypes.data}, {0: None, 1: None, 2: None, 3: None, 4: None, 5: None}):
            rc, res, dbuf, offs, _ = _read_dev(Z, torch, r, ents, caps, override=override)
            assert rc == 21, override
            assert res == [-1] * len(ents)                                             # rejected on the host: nothing ran, no result was written
            assert bool((dbuf == CANARY).all()) and bool((host == CANARY).all())
        # a destination that leaves its allocation: 2^40 bytes from inside a 4 KiB tensor
        small = torch.full((4096,), CANARY, dtype=torch.uint8, device="cuda:0")
        huge = list(caps); huge[3] = 1 << 40
        rc, res, dbuf, offs, _ = _read_dev(Z, torch, r, ents, huge, override={3: small.data_ptr() + 100}, room=caps)
        assert rc == 21 and res == [-1] * len(ents)
        assert bool((dbuf == CANARY).all()) and bool((small == CANARY).all())
        if torch.cuda.device_count() > 1:                                              # memory of another device than the batch's
            other = torch.full((max(caps) + 64,), CANARY, dtype=torch.uint8, device="cuda:1")
            torch.cuda.synchronize(1)
            rc, res, dbuf, offs, _ = _read_dev(Z, torch, r, ents, caps, override={4: other.data_ptr()})
            assert rc == 21 and res == [-1] * len(ents)
            assert bool((dbuf == CANARY).all()) and bool((other == CANARY).all())
        # no bytes at NULL and at a host address pass the rule: the call runs, that entry gets the verdict the host path gives it
        none = list(caps); none[2] = 0
        hrc, hres, _, hlast = _read_host(Z, r, ents, none)
        assert hrc == 0 and hres[2] != 0 and [v for k, v in enumerate(hres) if k != 2] == [0] * (len(ents) - 1)
        for at in (None, host.ctypes.data):
            rc, res, dbuf, offs, last = _read_dev(Z, torch, r, ents, none, override={2: at})
            assert (rc, res, last) == (hrc, hres, hlast)
            assert bool((host == CANARY).all())
        # the same batch with good pointers still reads
        assert _same_as_host(Z, torch, r, ents, caps) == [0] * len(ents)
    finally:
        Z.lib.zpack_close_reader(C.byref(r))


# ------------------------------------------------------------------------------------------------ writes

WRITE_SIZES = [0, 1, 65535, 65536, 65537, (2 << 20) + 17]


def _write(Z, torch, tmp_path, sink, files, method, level, on_device):
    """files: [(name, bytes)] -> archive bytes, the writer's entries, write_offset, rc"""
    w = Writer()
    path = str(tmp_path / ("dev.zpk" if on_device else "host.zpk"))
    assert (Z.lib.zpack_init_writer(C.byref(w), path.encode()) if sink == "file" else Z.lib.zpack_init_writer_heap(C.byref(w), 0)) == 0
    opts = CompressOptions(method, level)
    arr = (File * len(files))()
    keep = []
    if on_device:
        # sources at odd addresses inside one tensor, nothing behind the last one but the allocator's rounding
        pos, offs = 0, []
        for k, (_, data) in enumerate(files):
            pos = ((pos + 15) & ~15) + (k * 7 + 1) % 16
            offs.append(pos)
            pos += len(data)
        h = np.full(max(pos, 1), CANARY, dtype=np.uint8)
        for o, (_, data) in zip(offs, files):
            h[o:o + len(data)] = np.frombuffer(data, dtype=np.uint8)
        t = torch.from_numpy(h).to("cuda:0")
        torch.cuda.synchronize()
        keep.append(t)
    for k, (name, data) in enumerate(files):
        arr[k].filename = name.encode(); arr[k].size = len(data); arr[k].options = C.pointer(opts); arr[k].cctx = None
        if on_device:
            arr[k].buffer = C.cast(t.data_ptr() + offs[k], u8p) if len(data) else None
        else:
            b = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data if len(data) else b"\0")
            keep.append(b)
            arr[k].buffer = C.cast(b, u8p)
    assert Z.lib.zpack_write_header(C.byref(w)) == 0 and Z.lib.zpack_write_data_header(C.byref(w)) == 0
    rc = (Z.lib.zpack_amd_write_files_device if on_device else Z.lib.zpack_write_files)(C.byref(w), arr, len(files))
    table = [(w.file_entries[i].filename, w.file_entries[i].offset, w.file_entries[i].comp_size, w.file_entries[i].uncomp_size,
              w.file_entries[i].hash, w.file_entries[i].comp_method) for i in range(w.file_count)]
    at = (int(w.write_offset), int(w.last_return))
    assert Z.lib.zpack_write_cdr(C.byref(w)) == 0 and Z.lib.zpack_write_eocdr(C.byref(w)) == 0
    arc = bytes(C.cast(w.buffer, C.POINTER(C.c_uint8 * w.file_size)).contents) if sink == "heap" else None
    Z.lib.zpack_close_writer(C.byref(w))
    if sink == "file":
        arc = open(path, "rb").read()
    return arc, table, at, rc


@pytest.mark.parametrize("method,level", [(METHOD_NONE, 0), (METHOD_LZ4, 0), (METHOD_LZ4, 3), (METHOD_ZSTD, 0), (METHOD_ZSTD, 3)])
@pytest.mark.parametrize("sink", ["heap", "file"])
def test_written_archive_is_the_one_zpack_write_files_writes(Z, torch, tmp_path, method, level, sink):
    files = [("t%d" % k, _plain(3 * k if k != 2 else 1, n)) for k, n in enumerate(WRITE_SIZES)]      # (text; one of random bytes)
    harc, htable, hat, hrc = _write(Z, torch, tmp_path, sink, files, method, level, False)
    darc, dtable, dat, drc = _write(Z, torch, tmp_path, sink, files, method, level, True)
    assert hrc == 0 and drc == 0
    assert dtable == htable and dat == hat
    assert darc == harc
    o = oracle()
    ents = zpk.parse(darc)
    assert [e["filename"] for e in ents] == [n for n, _ in files]
    for e, (name, data) in zip(ents, files):
        assert e["uncomp_size"] == len(data) and e["hash"] == dg.xxh3(data) and e["method"] == method
        rc, out, got, h = o.entry_decode(darc, e["offset"], e["comp_size"], e["uncomp_size"], e["hash"], e["method"], len(data))
        assert rc == 0 and out == data, name


def test_write_pointer_check(Z, torch, tmp_path):
    host = np.zeros(4096, dtype=np.uint8)
    for ptr in (None, host.ctypes.data):
        w = Writer()
        assert Z.lib.zpack_init_writer_heap(C.byref(w), 0) == 0
        opts = CompressOptions(METHOD_LZ4, 0)
        good = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        arr = (File * 2)()
        arr[0].filename = b"good"; arr[0].buffer = C.cast(good.data_ptr(), u8p); arr[0].size = 4096; arr[0].options = C.pointer(opts)
        arr[1].filename = b"bad"; arr[1].buffer = C.cast(ptr, u8p) if ptr else None; arr[1].size = 4096; arr[1].options = C.pointer(opts)
        assert Z.lib.zpack_amd_write_files_device(C.byref(w), arr, 2) == 21
        assert w.file_count == 0 and w.write_offset == 0
        if ptr is None and torch.cuda.device_count() > 1:                              # memory of another device than the batch's
            other = torch.zeros(4096, dtype=torch.uint8, device="cuda:1")
            torch.cuda.synchronize(1)
            arr[1].buffer = C.cast(other.data_ptr(), u8p)
            assert Z.lib.zpack_amd_write_files_device(C.byref(w), arr, 2) == 21
            assert w.file_count == 0 and w.write_offset == 0
        # no bytes at that address pass the rule, and the next call on the same writer writes both files
        # (a source that leaves its allocation is checked where no scratch of its compress bound is asked for first: on a device sink,
        # test_gpu_device_sink.py::test_pointers_are_checked_on_the_host)
        arr[1].buffer = C.cast(ptr, u8p) if ptr else None; arr[1].size = 0
        assert Z.lib.zpack_amd_write_files_device(C.byref(w), arr, 2) == 0
        assert w.file_count == 2 and w.file_entries[0].uncomp_size == 4096 and w.file_entries[1].uncomp_size == 0
        Z.lib.zpack_close_writer(C.byref(w))


# ------------------------------------------------------------------------------------------------ the Python view

def test_device_io_round_trip(torch, tmp_path):
    from zpack_amd import device_io
    g = torch.Generator(device="cpu").manual_seed(5)
    tensors = {
        "w.f32": torch.randn(1000, 33, generator=g).to("cuda:0"),
        "idx.i64": torch.arange(70000, dtype=torch.int64, device="cuda:0"),
        "empty": torch.zeros(0, dtype=torch.uint8, device="cuda:0"),
        "one": torch.full((1,), 9, dtype=torch.uint8, device="cuda:0"),
        "mask.u8": (torch.arange(300001, device="cuda:0") % 7 == 0).to(torch.uint8),
    }
    path = str(tmp_path / "rt.zpk")
    for method, level in ((device_io.METHOD_LZ4, 0), (device_io.METHOD_ZSTD, 3), (device_io.METHOD_NONE, 0)):
        assert device_io.write_files_device(path, tensors, method=method, level=level) is None
        out, status = device_io.read_files_device(path)
        assert status == [0] * len(tensors) and len(out) == len(tensors)
        for (name, t), got in zip(tensors.items(), out):
            assert got.dtype == torch.uint8 and got.is_cuda and got.numel() == t.numel() * t.element_size()
            assert torch.equal(got, t.contiguous().reshape(-1).view(torch.uint8)), name
        some, st = device_io.read_files_device(open(path, "rb").read(), names=["one", "w.f32"])
        assert st == [0, 0] and torch.equal(some[1].view(torch.float32).reshape(1000, 33), tensors["w.f32"]) and int(some[0][0]) == 9
    heap = device_io.write_files_device(None, tensors, method=device_io.METHOD_LZ4, level=0)      # no path: the archive as bytes
    assert [e["filename"] for e in zpk.parse(heap)] == list(tensors)
    out, status = device_io.read_files_device(heap, names=["mask.u8"])
    assert status == [0] and torch.equal(out[0], tensors["mask.u8"])
