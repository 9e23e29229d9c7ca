"""GPU: a writer whose sink is an archive image in DEVICE memory (include/zpack_amd.h: zpack_amd_init_writer_device), every write call on
it, and the codec call behind the batch writes (zpk_codec_encode_batch_dsink: the frames encoded into the codec's staging and committed to
the sink by k_sink_cut / k_sink_place, sink_commit.h; the rules: dsink_plan.h).

The reference of every write is the same sequence of calls of the same library on a HEAP writer: the same return values, the same
last_return, the same entry table and offsets, and the same bytes in [0, write_offset).  Every sink lies between 256 guard bytes of 0xA5
on both sides, which are checked after every call.  Memory comes from torch."""
import ctypes as C

import numpy as np
import pytest

import zpack_amd
from benchdata import datagen as dg
from tests import zpk
from tests._libs import (Reader, Writer, File, FileEntry, Stream, CompressOptions, u8p, oracle, have_ref, ref,
                         METHOD_NONE, METHOD_ZSTD, METHOD_LZ4)
from tests.device_mem import torch, Z, _plain                                          # noqa: F401  (torch, Z: fixtures)

pytestmark = pytest.mark.gpu

PFE = C.POINTER(FileEntry)
OK, BUFFER_TOO_SMALL, COMPRESS_FAILED, STREAM_INVALID, NOT_AVAILABLE, NOT_OPENED = 0, 12, 14, 21, 24, 2
GUARD, FILL = 256, 0xA5
BIG = (2 << 20) + 17                             # the smallest entry written in pieces (ZPK_OPT_ENC_SPLIT_MIN: 2 MiB)
SIZES = [4095, 0, 1, 15, 16, 17, 65537, BIG]     # (the first file has bytes: "inside file 0" needs some)
KINDS = [(METHOD_NONE, 0), (METHOD_LZ4, 0), (METHOD_ZSTD, 1), (METHOD_ZSTD, 3)]


@pytest.fixture(scope="module")
def L():
    lib = zpack_amd.lib()
    vp, u64 = C.c_void_p, C.c_uint64
    lib.zpk_codec_encode_batch_host.argtypes = [vp, vp, vp, u64, vp, vp]
    return lib


# ------------------------------------------------------------------------------------------------ helpers

class Sink:
    """`capacity` bytes of device memory `shift` bytes behind 256 guard bytes, 256 more behind them; everything starts as 0xA5"""

    def __init__(self, torch, capacity, shift=0):
        self.torch, self.capacity, self.lo = torch, capacity, GUARD + shift
        self.t = torch.full((self.lo + capacity + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        self.ptr = self.t.data_ptr() + self.lo

    def guards_intact(self):
        self.torch.cuda.synchronize()
        return bool((self.t[:self.lo] == FILL).all()) and bool((self.t[self.lo + self.capacity:] == FILL).all())

    def bytes(self, n=None):
        self.torch.cuda.synchronize()
        n = self.capacity if n is None else n
        return self.t[self.lo:self.lo + n].cpu().numpy().tobytes()


def _file_array(torch, specs, on_device):
    """specs: [(name, plaintext, method, level)] -> the zpack_file array (host buffers, or device addresses at odd offsets of one tensor)"""
    arr = (File * max(len(specs), 1))()
    keep = []
    if on_device:
        pos, offs = 0, []
        for k, s in enumerate(specs):
            pos = ((pos + 15) & ~15) + (k * 7 + 1) % 16
            offs.append(pos)
            pos += len(s[1])
        h = np.full(max(pos, 1), 0x5C, dtype=np.uint8)
        for o, s in zip(offs, specs):
            h[o:o + len(s[1])] = np.frombuffer(s[1], dtype=np.uint8)
        t = torch.from_numpy(h).to("cuda:0")
        torch.cuda.synchronize()
        keep.append(t)
    for k, (name, data, method, level) in enumerate(specs):
        opts = CompressOptions(method, level)
        keep.append(opts)
        arr[k].filename = name.encode(); arr[k].size = len(data); arr[k].options = C.pointer(opts); arr[k].cctx = None
        if on_device:
            arr[k].buffer = C.cast(t.data_ptr() + offs[k], u8p) if len(data) else None
        else:
            b = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data if len(data) else b"\0")
            keep.append(b)
            arr[k].buffer = C.cast(b, u8p)
    return arr, keep


def _state(w):
    """everything of a writer that the contract says equals the heap writer's"""
    table = [(w.file_entries[i].filename, int(w.file_entries[i].offset), int(w.file_entries[i].comp_size), int(w.file_entries[i].uncomp_size),
              int(w.file_entries[i].hash), int(w.file_entries[i].comp_method)) for i in range(w.file_count)]
    return dict(table=table, file_count=int(w.file_count), write_offset=int(w.write_offset), file_size=int(w.file_size),
                cdr_offset=int(w.cdr_offset), eocdr_offset=int(w.eocdr_offset), last_return=int(w.last_return))


def _run(Z, sink, ops):
    """the calls `ops` (each a function of the writer -> return code) on a heap writer (sink None) or on a writer over `sink`
    -> (return codes, the writer's state behind every call, the bytes [0, file_size)); a device sink's guards are checked after every call"""
    w = Writer()
    if sink is None:
        assert Z.lib.zpack_init_writer_heap(C.byref(w), 0) == OK
    else:
        assert Z.lib.zpack_amd_init_writer_device(C.byref(w), sink.ptr, sink.capacity) == OK
        assert w.buffer is None or not w.buffer
        assert not w.file and sink.guards_intact()
    rcs, states = [], []
    for op in ops:
        rcs.append(op(w))
        states.append(_state(w))
        if sink is not None:
            assert sink.guards_intact(), "call %d wrote outside the sink" % len(rcs)
    n = int(w.file_size)
    data = bytes(C.cast(w.buffer, C.POINTER(C.c_uint8 * n)).contents) if sink is None and n else (sink.bytes(n) if sink is not None else b"")
    Z.lib.zpack_close_writer(C.byref(w))
    if sink is not None:
        assert sink.guards_intact()
    return rcs, states, data


def _archive_ops(Z, arr, n, on_device):
    write = Z.lib.zpack_amd_write_files_device if on_device else Z.lib.zpack_write_files
    return [lambda w: Z.lib.zpack_write_header(C.byref(w)), lambda w: Z.lib.zpack_write_data_header(C.byref(w)),
            lambda w: write(C.byref(w), arr, n), lambda w: Z.lib.zpack_write_cdr(C.byref(w)), lambda w: Z.lib.zpack_write_eocdr(C.byref(w))]


def _capacity(L, specs):
    """header + data signature + the compress bounds + CDR + EOCDR"""
    L.zpk_codec_compress_bound.restype = C.c_size_t
    return 10 + sum(int(L.zpk_codec_compress_bound(m, len(d))) for _, d, m, _ in specs) + 20 + sum(35 + len(n) for n, _, _, _ in specs) + 12


@pytest.fixture(scope="module")
def specs():
    """sizes 0, 1, 15, 16, 17, 4095, 65 537, 2 MiB + 17 in none, LZ4, Zstandard level 1 and level 3, and one incompressible LZ4 entry of
    70 000 random bytes: every size in every kind, 33 files"""
    out = []
    for k, (m, lv) in enumerate(KINDS):
        for j, n in enumerate(SIZES):
            out.append(("f%d_%d_%d" % (m, lv, n), _plain(3 * (k * len(SIZES) + j), n), m, lv))        # (text)
    out.append(("random70000", np.random.default_rng(70000).integers(0, 256, 70000, dtype=np.uint8).tobytes(), METHOD_LZ4, 0))
    return out


@pytest.fixture(scope="module")
def heap_run(Z, torch, specs):
    """the reference: the archive of `specs` on a heap writer, once for all tests -> (return codes, states, bytes)"""
    arr, keep = _file_array(torch, specs, False)
    return _run(Z, None, _archive_ops(Z, arr, len(specs), False))


# ------------------------------------------------------------------------------------------------ 1. identity

@pytest.mark.parametrize("on_device", [False, True], ids=["host_plaintext", "device_plaintext"])
@pytest.mark.parametrize("shift", [0, 1, 7, 15])
def test_the_image_is_the_heap_writers_archive(Z, L, torch, specs, heap_run, on_device, shift):
    hrcs, hstates, harc = heap_run
    assert hrcs == [OK] * 5
    if on_device:                                                                     # (the heap writer from device plaintext: the same archive)
        arr, keep = _file_array(torch, specs, True)
        rcs2, states2, arc2 = _run(Z, None, _archive_ops(Z, arr, len(specs), True))
        assert rcs2 == hrcs and states2 == hstates and arc2 == harc
    arr, keep = _file_array(torch, specs, on_device)
    sink = Sink(torch, _capacity(L, specs), shift)
    rcs, states, arc = _run(Z, sink, _archive_ops(Z, arr, len(specs), on_device))
    assert rcs == hrcs
    assert states == hstates                                                          # after every call: table, offsets, last_return
    assert arc == harc
    assert states[-1]["file_count"] == len(specs) and states[-1]["file_size"] == len(harc)


def test_zpack_write_archive_on_a_device_sink(Z, L, torch, specs, heap_run):
    arr, keep = _file_array(torch, specs, False)
    ops = [lambda w: Z.lib.zpack_write_archive(C.byref(w), arr, len(specs))]
    hrcs, hstates, harc = _run(Z, None, ops)
    assert hrcs == [OK] and harc == heap_run[2]
    rcs, states, arc = _run(Z, Sink(torch, _capacity(L, specs), 3), ops)
    assert rcs == hrcs and states == hstates and arc == harc


def test_the_writer_struct_and_its_record(Z, torch):
    sink = Sink(torch, 4096)
    w = Writer()
    p, cap, dev = C.c_void_p(1), C.c_size_t(7), C.c_int(7)
    assert Z.lib.zpack_amd_writer_device_image(C.byref(w), C.byref(p), C.byref(cap), C.byref(dev)) == OK and (p.value, cap.value, dev.value) == (None, 0, -1)
    assert Z.lib.zpack_write_header(C.byref(w)) == NOT_OPENED
    assert Z.lib.zpack_amd_init_writer_device(C.byref(w), sink.ptr, 4096) == OK
    assert not w.buffer and not w.file and w.write_offset == 0 and w.file_size == 0
    assert Z.lib.zpack_amd_writer_device_image(C.byref(w), C.byref(p), C.byref(cap), C.byref(dev)) == OK and (p.value, cap.value, dev.value) == (sink.ptr, 4096, 0)
    assert Z.lib.zpack_write_header(C.byref(w)) == OK and w.write_offset == 6
    Z.lib.zpack_close_writer(C.byref(w))
    assert bytes(w) == bytes(C.sizeof(Writer))
    assert Z.lib.zpack_amd_writer_device_image(C.byref(w), C.byref(p), C.byref(cap), C.byref(dev)) == OK and (p.value, cap.value, dev.value) == (None, 0, -1)
    assert Z.lib.zpack_write_header(C.byref(w)) == NOT_OPENED                        # the record went with the close; the image stays the caller's
    assert sink.guards_intact()
    # the struct serves again, as any kind
    assert Z.lib.zpack_init_writer_heap(C.byref(w), 0) == OK and Z.lib.zpack_write_header(C.byref(w)) == OK
    assert Z.lib.zpack_amd_writer_device_image(C.byref(w), C.byref(p), C.byref(cap), C.byref(dev)) == OK and p.value is None
    Z.lib.zpack_close_writer(C.byref(w))
    # a struct that was never closed and is zeroed: the record left at its address does not make it an opened writer
    assert Z.lib.zpack_amd_init_writer_device(C.byref(w), sink.ptr, 4096) == OK
    leaked_ctx = w.zstd_cctx
    C.memset(C.byref(w), 0, C.sizeof(Writer))
    assert leaked_ctx is None and Z.lib.zpack_write_header(C.byref(w)) == NOT_OPENED
    assert Z.lib.zpack_amd_init_writer_device(C.byref(w), sink.ptr + 16, 100) == OK   # ... and the next init there replaces it
    assert Z.lib.zpack_amd_writer_device_image(C.byref(w), C.byref(p), C.byref(cap), C.byref(dev)) == OK and (p.value, cap.value) == (sink.ptr + 16, 100)
    Z.lib.zpack_close_writer(C.byref(w))


# ------------------------------------------------------------------------------------------------ 2. round trip without the host

def test_round_trip_on_the_device_and_through_the_checkers(Z, L, torch, specs, heap_run):
    arr, keep = _file_array(torch, specs, True)
    sink = Sink(torch, _capacity(L, specs), 5)
    rcs, states, arc = _run(Z, sink, _archive_ops(Z, arr, len(specs), True))
    assert rcs == [OK] * 5 and arc == heap_run[2]
    size = states[-1]["file_size"]
    # read where it was written: a reader over the sink, plaintext into device tensors
    r = Reader()
    assert Z.lib.zpack_amd_init_reader_device(C.byref(r), sink.ptr, size) == OK
    n = int(r.file_count)
    assert n == len(specs)
    outs = [torch.full((max(len(s[1]), 1) + 32,), FILL, dtype=torch.uint8, device="cuda:0") for s in specs]
    torch.cuda.synchronize()
    res = (C.c_int * n)(*([-1] * n))
    rc = Z.lib.zpack_amd_read_files_device(C.byref(r), (PFE * n)(*[C.pointer(r.file_entries[i]) for i in range(n)]), n,
                                           (C.c_void_p * n)(*[o.data_ptr() + 16 for o in outs]), (C.c_size_t * n)(*[len(s[1]) for s in specs]), res, None)
    torch.cuda.synchronize()
    assert rc == OK and list(res) == [OK] * n
    for o, (name, data, m, lv) in zip(outs, specs):
        got = o.cpu().numpy()
        assert got[16:16 + len(data)].tobytes() == data, name
        assert (got[:16] == FILL).all() and (got[16 + len(data):] == FILL).all(), name
    Z.lib.zpack_close_reader(C.byref(r))
    assert sink.guards_intact()
    # the fetched image, entry for entry through the oracle and, where it was built, through the compiled reference
    o = oracle()
    ents = zpk.parse(arc)
    assert [e["filename"] for e in ents] == [s[0] for s in specs]
    for e, (name, data, m, lv) in zip(ents, specs):
        assert e["uncomp_size"] == len(data) and e["hash"] == dg.xxh3(data) and e["method"] == m
        rc, out, got, h = o.entry_decode(arc, e["offset"], e["comp_size"], e["uncomp_size"], e["hash"], e["method"], len(data))
        assert rc == 0 and out == data, name
    if have_ref():
        rz = ref()
        rc, rr, keep2 = rz.open_memory(arc)
        assert rc == 0 and rr.file_count == len(specs)
        for i, (name, data, m, lv) in enumerate(specs):
            rc, out = rz.read_file(rr, i, len(data))
            assert rc == 0 and out == data, name
        rz.close_reader(rr)


# ------------------------------------------------------------------------------------------------ 3. a full sink

def _model(table, capacity, at=10):
    """the append rule over the heap writer's table: the files in front of the first one that does not end inside the sink"""
    placed = 0
    for name, offset, comp, uncomp, h, m in table:
        if offset + comp > capacity:
            break
        placed += 1
        at = offset + comp
    return placed, at


@pytest.mark.parametrize("on_device", [False, True], ids=["host_plaintext", "device_plaintext"])
@pytest.mark.parametrize("case", ["ends_at_file_k", "one_byte_short", "inside_file_0", "no_room_for_the_cdr", "no_room_for_the_header"])
def test_a_full_sink_takes_the_files_in_front_of_the_one_that_does_not_fit(Z, L, torch, specs, heap_run, case, on_device):
    hrcs, hstates, harc = heap_run
    table, cdr_at = hstates[-1]["table"], hstates[-1]["cdr_offset"]
    k = 14                                                                            # a file with bytes whose successor has bytes too
    assert table[k][2] > 0 and table[k + 1][2] > 0 and table[0][2] > 1
    capacity = {"ends_at_file_k": table[k][1] + table[k][2], "one_byte_short": table[k][1] + table[k][2] - 1,
                "inside_file_0": 10 + table[0][2] // 2, "no_room_for_the_cdr": cdr_at + 5, "no_room_for_the_header": 3}[case]
    arr, keep = _file_array(torch, specs, on_device)
    sink = Sink(torch, capacity, 9)
    rcs, states, arc = _run(Z, sink, _archive_ops(Z, arr, len(specs), on_device))
    if case == "no_room_for_the_header":
        assert rcs[:2] == [BUFFER_TOO_SMALL, BUFFER_TOO_SMALL] and states[1]["write_offset"] == 0 and states[1]["file_size"] == 0
        assert rcs[2] == BUFFER_TOO_SMALL and states[2]["file_count"] == 0 and states[2]["write_offset"] == 0
        assert states[2]["last_return"] == table[0][2]                                # the first file's comp_size: it was compressed, and did not fit
        assert sink.bytes() == bytes([FILL]) * capacity
        return
    assert rcs[:2] == [OK, OK]
    placed, at = _model(table, capacity)
    assert placed == {"ends_at_file_k": k + 1, "one_byte_short": k, "inside_file_0": 0, "no_room_for_the_cdr": len(specs)}[case]
    s = states[2]
    if placed == len(specs):
        assert rcs[2] == OK and s == hstates[2]
    else:
        assert rcs[2] == BUFFER_TOO_SMALL
        assert s["last_return"] == table[placed][2]                                   # that file's comp_size
    assert s["file_count"] == placed and s["table"] == table[:placed]
    assert s["write_offset"] == at and s["file_size"] == at
    assert sink.bytes(at) == harc[:at]
    # the fixed blocks behind the files: one that fits is written where the files ended, one that does not writes nothing and the
    # offsets do not move
    cdr_size = 20 + sum(35 + len(row[0]) for row in table[:placed])
    for i, size, field in ((3, cdr_size, "cdr_offset"), (4, 12, "eocdr_offset")):
        if capacity - at >= size:
            assert rcs[i] == OK and states[i][field] == at and states[i]["write_offset"] == at + size
            at += size
        else:
            assert rcs[i] == BUFFER_TOO_SMALL and states[i][field] == 0 and states[i]["write_offset"] == at and states[i]["file_size"] == at
        assert states[i]["file_count"] == placed
    if case in ("ends_at_file_k", "no_room_for_the_cdr"):
        assert rcs[3:] == [BUFFER_TOO_SMALL, BUFFER_TOO_SMALL]
    assert len(arc) == at and arc[:states[2]["write_offset"]] == harc[:states[2]["write_offset"]]


# ------------------------------------------------------------------------------------------------ 4. the cut in the codec

def _codec_batch(L, rows):
    """rows: [(plaintext, method, level, dst_capacity or None)] -> (sources, descriptors)"""
    L.zpk_codec_compress_bound.restype = C.c_size_t
    srcs = [np.frombuffer(d, dtype=np.uint8) if len(d) else np.zeros(0, dtype=np.uint8) for d, _, _, _ in rows]
    desc = np.zeros(len(rows), dtype=zpack_amd.ENCODE_DESC)
    for i, (d, m, lv, cap) in enumerate(rows):
        desc[i]["size"] = len(d); desc[i]["method"] = m; desc[i]["level"] = lv
        desc[i]["dst_capacity"] = int(L.zpk_codec_compress_bound(m, len(d))) if cap is None else cap
    return srcs, desc


def _encode_host(L, codec, srcs, desc):
    """zpk_codec_encode_batch_host -> (results, [frame bytes])"""
    n = len(desc)
    keep = [np.ascontiguousarray(s) for s in srcs]
    outs = [np.zeros(int(d["dst_capacity"]) + 16, dtype=np.uint8) for d in desc]
    res = np.zeros(n, dtype=zpack_amd.ENCODE_RESULT)
    rc = L.zpk_codec_encode_batch_host(codec.h, (C.c_void_p * n)(*[a.ctypes.data if a.size else None for a in keep]), desc.ctypes.data, n,
                                       (C.c_void_p * n)(*[o.ctypes.data for o in outs]), res.ctypes.data)
    assert rc == 0, rc
    return res, [o[:int(r["comp_size"])].tobytes() if r["status"] == 0 else b"" for o, r in zip(outs, res)]


@pytest.fixture(scope="module")
def codec_rows():
    sizes = [300, 0, 70000, 16384, 16385, 1, BIG, 5000, 33000, 100, 0, 65536]
    return [(_plain(3 * i, n), (METHOD_LZ4, METHOD_ZSTD, METHOD_NONE)[i % 3], 1, None) for i, n in enumerate(sizes)]


@pytest.mark.parametrize("src_on_device", [False, True], ids=["host_sources", "device_sources"])
@pytest.mark.parametrize("why", ["capacity", "room", "room_exact", "none"])
def test_the_cut_in_the_codec(L, torch, codec_rows, why, src_on_device):
    codec = zpack_amd.Codec(0)
    j = 7
    rows = list(codec_rows)
    if why == "capacity":                                                             # a dst_capacity too small for entry j: its status stops the batch
        rows[j] = (rows[j][0], rows[j][1], rows[j][2], 40)
    srcs, desc = _codec_batch(L, rows)
    want, frames = _encode_host(L, codec, srcs, desc)
    offs = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int64)
    total = int(offs[-1])
    if why == "capacity":
        assert want[j]["status"] in (BUFFER_TOO_SMALL, COMPRESS_FAILED)
        room, cut = total + 100, j
    elif why == "room":
        room, cut = int(offs[j]) + len(frames[j]) - 1, j                              # one byte short of entry j's end
    elif why == "room_exact":
        room, cut = int(offs[j + 1]), j + 1                                           # entry j ends where the room ends; j + 1 has bytes
        assert len(frames[j + 1]) > 0
    else:
        room, cut = total, len(rows)
    sink = Sink(torch, total + 4096, 11)                                              # the allocation is larger than the room: behind the cut it keeps its fill
    if src_on_device:
        dev = [torch.from_numpy(s.copy()).to("cuda:0") if s.size else None for s in srcs]
        torch.cuda.synchronize()
        given = [t.data_ptr() if t is not None else None for t in dev]
    else:
        given = srcs
    res, placed, nbytes = codec.encode_batch_dsink(given, desc, sink.t, sink_offset=sink.lo, room=room, src_on_device=src_on_device)
    assert placed == cut and nbytes == int(offs[cut])
    upto = min(cut + 1, len(rows))
    for f in ("status", "detail", "comp_size", "hash"):
        assert np.array_equal(res[f][:upto], want[f][:upto]), f
    got = sink.bytes()
    assert got[:nbytes] == b"".join(frames[:cut])
    assert got[nbytes:] == bytes([FILL]) * (len(got) - nbytes)                        # nothing at or behind offsets[f]: stricter than the library's contract
    assert sink.guards_intact()
    assert codec.dsink_stats()["sub_batches"] == 1
    codec.close()


def test_sub_batches_land_behind_each_other(L, torch, codec_rows):
    codec = zpack_amd.Codec(0)
    srcs, desc = _codec_batch(L, codec_rows)
    want, frames = _encode_host(L, codec, srcs, desc)
    total = sum(len(f) for f in frames)
    codec.set_option(zpack_amd.OPT_DIMAGE_CHUNK, 100000)                              # staging slots per sub-batch: the 2 MiB entry goes alone
    for room, cut in ((total, len(frames)), (total - 1, len(frames) - 1), (sum(len(f) for f in frames[:7]) - 1, 6)):
        sink = Sink(torch, total + 512, 2)
        res, placed, nbytes = codec.encode_batch_dsink(srcs, desc, sink.t, sink_offset=sink.lo, room=room)
        assert codec.dsink_stats()["sub_batches"] >= (4 if cut >= len(frames) - 1 else 2)
        assert placed == cut and nbytes == sum(len(f) for f in frames[:cut])
        got = sink.bytes()
        assert got[:nbytes] == b"".join(frames[:cut]) and got[nbytes:] == bytes([FILL]) * (len(got) - nbytes)
        upto = min(cut + 1, len(frames))
        assert np.array_equal(res["comp_size"][:upto], want["comp_size"][:upto]) and np.array_equal(res["hash"][:upto], want["hash"][:upto])
        assert sink.guards_intact()
    codec.close()


# ------------------------------------------------------------------------------------------------ 5. ragged

def test_a_ragged_batch_in_one_call(Z, L, torch):
    """3000 entries of 0..300 bytes around one 4 MiB entry: more spans than waves in the grid's first round for the large entry's
    share, entries without bytes, entries of a few bytes — one call, one sub-batch"""
    rng = np.random.default_rng(33)
    sizes = [int(x) for x in rng.integers(1, 301, 3000)]
    for i in range(0, 3000, 97):
        sizes[i] = 0
    sizes.insert(1500, 4 << 20)
    specs = [("r%04d" % i, _plain(3 * i if i != 1500 else 0, n), (METHOD_LZ4, METHOD_NONE, METHOD_ZSTD)[i % 3], 1) for i, n in enumerate(sizes)]
    arr, keep = _file_array(torch, specs, False)
    ops = _archive_ops(Z, arr, len(specs), False)
    hrcs, hstates, harc = _run(Z, None, ops)
    assert hrcs == [OK] * 5
    rcs, states, arc = _run(Z, Sink(torch, _capacity(L, specs), 13), ops)
    assert rcs == hrcs and states[-1] == hstates[-1] and states[2] == hstates[2]
    assert arc == harc


# ------------------------------------------------------------------------------------------------ 6. raw copy

@pytest.mark.parametrize("source", ["device_image", "memory"])
def test_raw_copy_between_archives(Z, torch, heap_run, source):
    harc = heap_run[2]
    keep = (C.c_uint8 * len(harc)).from_buffer_copy(harc)
    rm = Reader()
    assert Z.lib.zpack_init_reader_memory_shared(C.byref(rm), C.cast(keep, u8p), len(harc)) == OK
    n = int(rm.file_count)
    picks = [i for i in range(n) if i % 3 != 1]                                       # entries with gaps between them, in archive order
    ents_m = (FileEntry * len(picks))(*[rm.file_entries[i] for i in picks])
    ops_m = [lambda w: Z.lib.zpack_write_header(C.byref(w)), lambda w: Z.lib.zpack_write_data_header(C.byref(w)),
             lambda w: Z.lib.zpack_write_files_from_archive(C.byref(w), C.byref(rm), ents_m, len(picks)),
             lambda w: Z.lib.zpack_write_cdr(C.byref(w)), lambda w: Z.lib.zpack_write_eocdr(C.byref(w))]
    hrcs, hstates, want = _run(Z, None, ops_m)
    assert hrcs == [OK] * 5 and hstates[-1]["file_count"] == len(picks)
    if source == "device_image":
        image = torch.from_numpy(np.frombuffer(harc, dtype=np.uint8).copy()).to("cuda:0")
        torch.cuda.synchronize()
        rd = Reader()
        assert Z.lib.zpack_amd_init_reader_device(C.byref(rd), image.data_ptr(), len(harc)) == OK
        ents_d = (FileEntry * len(picks))(*[rd.file_entries[i] for i in picks])
        ops = list(ops_m)
        ops[2] = lambda w: Z.lib.zpack_write_files_from_archive(C.byref(w), C.byref(rd), ents_d, len(picks))
    else:
        ops = ops_m
    rcs, states, got = _run(Z, Sink(torch, len(want) + 77, 6), ops)
    assert rcs == hrcs and states == hstates and got == want
    # an entry that does not fit: the ones in front of it are copied and entered, nothing of it is written
    t = hstates[2]["table"]
    capacity = t[5][1] + t[5][2] - 1
    rcs, states, got = _run(Z, Sink(torch, capacity, 6), ops[:3])
    assert rcs == [OK, OK, BUFFER_TOO_SMALL] and states[2]["file_count"] == 5 and states[2]["write_offset"] == t[5][1] and states[2]["table"] == t[:5]
    assert got == want[:t[5][1]]
    if source == "device_image":
        Z.lib.zpack_close_reader(C.byref(rd))
    Z.lib.zpack_close_reader(C.byref(rm))


# ------------------------------------------------------------------------------------------------ 7. streaming

@pytest.mark.parametrize("method,level", [(METHOD_LZ4, 0), (METHOD_ZSTD, 1), (METHOD_NONE, 0)])
def test_stream_writer_into_a_device_sink(Z, L, torch, method, level):
    size, window = 3 << 20, 64 << 10
    plain = np.frombuffer(_plain(0, size), dtype=np.uint8).copy()
    opts = CompressOptions(method, level)
    out_size = Z.lib.zpack_get_cstream_out_size(method)

    def stream_entry(w):
        st = Stream()
        assert Z.lib.zpack_init_stream(C.byref(st)) == OK
        out_buf = (C.c_uint8 * out_size)()
        st.next_out = C.cast(out_buf, u8p); st.avail_out = out_size
        Z.lib.zpack_reset_stream(C.byref(st))
        rc, pos = OK, 0
        while pos < size and rc == OK:
            n = min(window, size - pos)
            st.next_in = C.cast(plain.ctypes.data + pos, u8p); st.avail_in = n
            rc = Z.lib.zpack_write_file_stream(C.byref(w), C.byref(opts), C.byref(st), None)
            pos += n
        if rc == OK:
            rc = Z.lib.zpack_write_file_stream_end(C.byref(w), b"streamed", C.byref(opts), C.byref(st), None)
        Z.lib.zpack_close_stream(C.byref(st))
        return rc

    ops = [lambda w: Z.lib.zpack_write_header(C.byref(w)), lambda w: Z.lib.zpack_write_data_header(C.byref(w)), stream_entry,
           lambda w: Z.lib.zpack_write_cdr(C.byref(w)), lambda w: Z.lib.zpack_write_eocdr(C.byref(w))]
    hrcs, hstates, harc = _run(Z, None, ops)
    assert hrcs == [OK] * 5 and hstates[-1]["table"][0][3] == size
    rcs, states, arc = _run(Z, Sink(torch, len(harc) + 100, 4), ops)
    assert rcs == hrcs and states == hstates and arc == harc
    # a window that does not fit: BUFFER_TOO_SMALL, and nothing outside the sink
    rcs, states, arc = _run(Z, Sink(torch, len(harc) // 2, 4), ops[:3])
    assert rcs == [OK, OK, BUFFER_TOO_SMALL] and states[2]["write_offset"] <= len(harc) // 2 and arc == harc[:states[2]["write_offset"]]


# ------------------------------------------------------------------------------------------------ 8. pointers

def test_pointers_are_checked_on_the_host(Z, torch):
    host = np.full(8192, 0x3C, dtype=np.uint8)
    w = Writer()
    assert Z.lib.zpack_amd_init_writer_device(C.byref(w), host.ctypes.data, 4096) == STREAM_INVALID          # host memory as d_image
    assert bytes(w) == bytes(C.sizeof(Writer)) and Z.lib.zpack_write_header(C.byref(w)) == NOT_OPENED
    assert (host == 0x3C).all()
    t = torch.full((4096,), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert Z.lib.zpack_amd_init_writer_device(C.byref(w), t.data_ptr(), 1 << 40) == STREAM_INVALID           # a capacity that leaves the allocation
    assert Z.lib.zpack_amd_init_writer_device(C.byref(w), t.data_ptr() + 100, (1 << 40) - 100) == STREAM_INVALID
    assert bytes(w) == bytes(C.sizeof(Writer))
    assert Z.lib.zpack_amd_init_writer_device(None, t.data_ptr(), 4096) == STREAM_INVALID
    assert Z.lib.zpack_amd_init_writer_device(C.byref(w), None, 4096) == STREAM_INVALID
    # device plaintext handed to zpack_write_files as a host array: turned down before anything runs, nothing written
    sink = Sink(torch, 1 << 16)
    assert Z.lib.zpack_amd_init_writer_device(C.byref(w), sink.ptr, sink.capacity) == OK
    assert Z.lib.zpack_write_header(C.byref(w)) == OK and Z.lib.zpack_write_data_header(C.byref(w)) == OK
    before = sink.bytes()
    opts = CompressOptions(METHOD_LZ4, 0)
    hostbuf = (C.c_uint8 * 4096)()
    arr = (File * 2)()
    arr[0].filename = b"host"; arr[0].buffer = C.cast(hostbuf, u8p); arr[0].size = 4096; arr[0].options = C.pointer(opts)
    arr[1].filename = b"device"; arr[1].buffer = C.cast(t.data_ptr(), u8p); arr[1].size = 4096; arr[1].options = C.pointer(opts)
    assert Z.lib.zpack_write_files(C.byref(w), arr, 2) == STREAM_INVALID
    assert w.file_count == 0 and w.write_offset == 10 and sink.bytes() == before and sink.guards_intact()
    # host memory (and NULL with bytes) handed to zpack_amd_write_files_device
    arr[1].buffer = C.cast(hostbuf, u8p); arr[0].buffer = C.cast(t.data_ptr(), u8p)
    assert Z.lib.zpack_amd_write_files_device(C.byref(w), arr, 2) == STREAM_INVALID
    arr[1].buffer = None
    assert Z.lib.zpack_amd_write_files_device(C.byref(w), arr, 2) == STREAM_INVALID
    # ... a source that leaves its allocation, and, on a box with two cards, memory of another device than the sink's
    arr[1].buffer = C.cast(t.data_ptr() + 100, u8p); arr[1].size = 1 << 40
    assert Z.lib.zpack_amd_write_files_device(C.byref(w), arr, 2) == STREAM_INVALID
    arr[1].size = 4096
    if torch.cuda.device_count() > 1:
        other = torch.zeros(4096, dtype=torch.uint8, device="cuda:1")
        torch.cuda.synchronize(1)
        arr[1].buffer = C.cast(other.data_ptr(), u8p)
        assert Z.lib.zpack_amd_write_files_device(C.byref(w), arr, 2) == STREAM_INVALID
    assert w.file_count == 0 and w.write_offset == 10 and sink.bytes() == before and sink.guards_intact()
    # ... and the writer is still good
    arr[1].buffer = C.cast(t.data_ptr() + 1, u8p); arr[1].size = 4095
    assert Z.lib.zpack_amd_write_files_device(C.byref(w), arr, 2) == OK and w.file_count == 2
    # no bytes pass wherever they point: NULL and a host address, from device and from host plaintext
    arr[1].size = 0
    for k, (at, write) in enumerate(((None, Z.lib.zpack_amd_write_files_device), (C.cast(hostbuf, u8p), Z.lib.zpack_amd_write_files_device),
                                     (C.cast(t.data_ptr(), u8p), Z.lib.zpack_write_files))):
        arr[1].buffer = at
        if write is Z.lib.zpack_write_files:
            arr[0].buffer = C.cast(hostbuf, u8p)
        assert write(C.byref(w), arr, 2) == OK and w.file_count == 4 + 2 * k
    assert sink.guards_intact()
    Z.lib.zpack_close_writer(C.byref(w))
    assert sink.guards_intact()


def test_a_sink_on_another_device_than_the_plaintext(Z, torch):
    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    sink = torch.full((1 << 16,), FILL, dtype=torch.uint8, device="cuda:1")
    plain = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize(0); torch.cuda.synchronize(1)
    w = Writer()
    assert Z.lib.zpack_amd_init_writer_device(C.byref(w), sink.data_ptr(), sink.numel()) == OK
    opts = CompressOptions(METHOD_LZ4, 0)
    arr = (File * 1)()
    arr[0].filename = b"x"; arr[0].buffer = C.cast(plain.data_ptr(), u8p); arr[0].size = 4096; arr[0].options = C.pointer(opts)
    rc = Z.lib.zpack_amd_write_files_device(C.byref(w), arr, 1)
    assert rc in (STREAM_INVALID, NOT_AVAILABLE)                                      # NOT_AVAILABLE: the writer's context (ZPACK_AMD_DEVICES) has no codec on the sink's device
    assert w.file_count == 0 and w.write_offset == 0
    Z.lib.zpack_close_writer(C.byref(w))


# ------------------------------------------------------------------------------------------------ the Python view

def test_write_archive_device_round_trip(torch):
    from zpack_amd import device_io
    g = torch.Generator(device="cpu").manual_seed(6)
    tensors = {
        "w.f32": torch.randn(700, 33, generator=g).to("cuda:0"),
        "empty": torch.zeros(0, dtype=torch.uint8, device="cuda:0"),
        "idx.i64": torch.arange(50000, dtype=torch.int64, device="cuda:0"),
        "mask.u8": (torch.arange(300001, device="cuda:0") % 7 == 0).to(torch.uint8),
    }
    for method, level in ((device_io.METHOD_LZ4, 0), (device_io.METHOD_ZSTD, 1), (device_io.METHOD_NONE, 0)):
        image = device_io.write_archive_device(tensors, method=method, level=level)
        assert image.is_cuda and image.dtype == torch.uint8
        assert image.cpu().numpy().tobytes() == device_io.write_files_device(None, tensors, method=method, level=level)
        out, status = device_io.read_files_device(image)
        assert status == [0] * len(tensors)
        for (name, t), got in zip(tensors.items(), out):
            assert torch.equal(got, t.contiguous().reshape(-1).view(torch.uint8)), name
    with pytest.raises(RuntimeError):
        device_io.write_archive_device(tensors, capacity=1000)
