"""GPU: byte-plane entries through the library (include/zpack_amd.h: zpack_amd_write_files_device_planes, zpack_amd_read_files_device_planes),
the codec calls behind them and the torch view (zpack_amd/device_io.py), for LZ4 and Zstandard level 1.

The archive: bf16, fp32 and fp64 tensors of 1, 7, 4 096 and 65 537 elements, one uint8 entry with element size 1, one empty entry, one
entry with a tail (1 003 bytes, element size 4) and one bf16 entry of 3 MiB, which is written in pieces and read block-parallel.  The
reference of every write is zpack_amd_write_files_device from device buffers that hold the numpy-grouped bytes: the same image byte for
byte.  The reference of every read is zpack_amd_read_files_device of the same entries: the same results, return value and last_return,
and the bytes are the join of the bytes it delivers — or the 0xA5 the buffer held, with 64 canary bytes around every destination."""
import ctypes as C

import numpy as np
import pytest

import zpack_amd
from zpack_amd import device_io
from tests._libs import Reader, Writer, File, FileEntry, CompressOptions, u8p, oracle, have_ref, ref, METHOD_ZSTD, METHOD_LZ4
from tests.device_mem import torch, Z, _layout, CANARY, GAP            # noqa: F401  (torch, Z: fixtures)

pytestmark = pytest.mark.gpu

PFE = C.POINTER(FileEntry)
OK, HASH_MISMATCH, STREAM_INVALID = 0, 15, 21
MIS = (0, 3, 1, 15)
METHODS = [pytest.param((METHOD_LZ4, 0), id="lz4"), pytest.param((METHOD_ZSTD, 1), id="zstd1")]


def grouped(a, k):
    a = np.asarray(a, dtype=np.uint8)
    m = a.size // k
    return np.concatenate([a[:m * k].reshape(m, k).T.reshape(-1), a[m * k:]])


@pytest.fixture(scope="module")
def P(Z):
    """the library with the prototypes of the two new calls"""
    L = Z.lib
    R, W, vp, u64 = C.POINTER(Reader), C.POINTER(Writer), C.c_void_p, C.c_uint64
    L.zpack_amd_write_files_device_planes.argtypes = [W, C.POINTER(File), u64, C.POINTER(C.c_uint8)]
    L.zpack_amd_read_files_device_planes.argtypes = [R, C.POINTER(PFE), u64, vp, C.POINTER(C.c_size_t), C.POINTER(C.c_uint8), C.POINTER(C.c_int), vp]
    L.zpack_amd_test_files.argtypes = [R, C.POINTER(PFE), u64, C.POINTER(C.c_int), vp]
    return Z


@pytest.fixture(scope="module")
def plain(torch):
    """[(name, element size, the tensor's bytes as np.uint8)], computed once: the tensors are randn * 0.02, seeded"""
    g = torch.Generator().manual_seed(28)
    out = []
    for dt, k, tag in ((torch.bfloat16, 2, "bf16"), (torch.float32, 4, "fp32"), (torch.float64, 8, "fp64")):
        for n in (1, 7, 4096, 65537):
            t = (torch.randn(n, generator=g, dtype=torch.float32) * 0.02).to(dt)
            out.append(("%s_%d" % (tag, n), k, t.view(torch.uint8).numpy().copy()))
    rng = np.random.default_rng(28)
    out.append(("bytes", 1, np.frombuffer((b"the quick brown fox jumps over the lazy dog. " * 120)[:5001], dtype=np.uint8).copy()))
    out.append(("empty", 2, np.zeros(0, dtype=np.uint8)))
    out.append(("tail", 4, rng.integers(0, 256, 1003, dtype=np.uint8)))
    big = (torch.randn(3 << 19, generator=g, dtype=torch.float32) * 0.02).to(torch.bfloat16)
    out.append(("big_bf16", 2, big.view(torch.uint8).numpy().copy()))
    assert out[-1][2].size == 3 << 20
    return out


def _on_device(torch, arrays, mis=MIS):
    """the arrays back to back in one device buffer at misaligned addresses -> (buffer, [address or None])"""
    offs, total = _layout([a.size for a in arrays], mis)
    h = np.full(total, CANARY, dtype=np.uint8)
    for a, o in zip(arrays, offs):
        h[o:o + a.size] = a
    buf = torch.from_numpy(h).to("cuda:0")
    torch.cuda.synchronize()
    return buf, [buf.data_ptr() + o if a.size else None for a, o in zip(arrays, offs)], h


def _write(P, torch, names, arrays, mc, elem, sink, call="planes"):
    """header, data signature, the entries out of device memory, CDR, EOCDR -> (rc of the files call, the image's bytes, the entries'
    (offset, comp_size, uncomp_size, hash, method), write_offset behind the files call, the sources as they are afterwards == before)"""
    L = P.lib
    buf, addr, before = _on_device(torch, arrays)
    opts = CompressOptions(*mc)
    arr = (File * len(names))()
    for i, (nm, a) in enumerate(zip(names, arrays)):
        arr[i].filename = nm.encode()
        arr[i].buffer = C.cast(C.c_void_p(addr[i]), u8p)
        arr[i].size = a.size
        arr[i].options = C.pointer(opts)
        arr[i].cctx = None
    w = Writer()
    image_t = None
    if sink == "heap":
        assert L.zpack_init_writer_heap(C.byref(w), 0) == 0
    else:
        cap = device_io.archive_capacity([a.size for a in arrays], names, mc[0])
        image_t = torch.full((cap,), CANARY, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        assert L.zpack_amd_init_writer_device(C.byref(w), image_t.data_ptr(), cap) == 0
    try:
        assert L.zpack_write_header(C.byref(w)) == 0 and L.zpack_write_data_header(C.byref(w)) == 0
        at0 = int(w.write_offset)
        if call == "planes":
            rc = L.zpack_amd_write_files_device_planes(C.byref(w), arr, len(names), None if elem is None else (C.c_uint8 * len(names))(*elem))
        else:
            rc = L.zpack_amd_write_files_device(C.byref(w), arr, len(names))
        at1 = int(w.write_offset)
        ents = [(int(e.offset), int(e.comp_size), int(e.uncomp_size), int(e.hash), int(e.comp_method)) for e in (w.file_entries[i] for i in range(w.file_count))]
        assert L.zpack_write_cdr(C.byref(w)) == 0 and L.zpack_write_eocdr(C.byref(w)) == 0
        torch.cuda.synchronize()
        image = C.string_at(w.buffer, w.file_size) if sink == "heap" else image_t[:int(w.file_size)].cpu().numpy().tobytes()
        assert np.array_equal(buf.cpu().numpy(), before)                                # the sources are read, never written
        return rc, image, ents, (at0, at1)
    finally:
        L.zpack_close_writer(C.byref(w))


@pytest.fixture(scope="module", params=METHODS)
def made(request, P, torch, plain):
    """one method: the image written by the planes call into a heap writer, its entries, and everything the tests share"""
    mc = request.param
    names, elem, arrays = [p[0] for p in plain], [p[1] for p in plain], [p[2] for p in plain]
    rc, image, ents, _ = _write(P, torch, names, arrays, mc, elem, "heap")
    assert rc == OK and len(ents) == len(names)
    return dict(mc=mc, names=names, elem=elem, arrays=arrays, stored=[grouped(a, k) for a, k in zip(arrays, elem)], image=image, ents=ents)


class Opened:
    """a reader over the image: in host memory, or in device memory"""
    def __init__(self, P, torch, image, where):
        self.L, self.r = P.lib, Reader()
        if where == "memory":
            self.keep = (C.c_uint8 * len(image)).from_buffer_copy(image)
            assert self.L.zpack_init_reader_memory_shared(C.byref(self.r), C.cast(self.keep, u8p), len(image)) == 0
        else:
            self.keep = torch.from_numpy(np.frombuffer(image, dtype=np.uint8).copy()).to("cuda:0")
            torch.cuda.synchronize()
            assert self.L.zpack_amd_init_reader_device(C.byref(self.r), self.keep.data_ptr(), len(image)) == 0
        self.ents = [self.r.file_entries[i] for i in range(self.r.file_count)]

    def close(self):
        self.L.zpack_close_reader(C.byref(self.r))


def _read(P, torch, o, ents, caps, elem, call="planes"):
    """-> (rc, results, last_return), the whole device buffer as it is afterwards, the destinations' offsets"""
    n = len(ents)
    offs, total = _layout(caps, MIS)
    buf = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    addr = (C.c_void_p * n)(*[buf.data_ptr() + x for x in offs])
    ptrs = (PFE * n)(*[C.pointer(e) for e in ents])
    res = (C.c_int * n)(*([-1] * n))
    csz = (C.c_size_t * n)(*caps)
    if call == "planes":
        rc = P.lib.zpack_amd_read_files_device_planes(C.byref(o.r), ptrs, n, addr, csz, None if elem is None else (C.c_uint8 * n)(*elem), res, None)
    else:
        rc = P.lib.zpack_amd_read_files_device(C.byref(o.r), ptrs, n, addr, csz, res, None)
    torch.cuda.synchronize()
    return (rc, list(res), int(o.r.last_return)), buf.cpu().numpy(), offs


def _want(total, offs, arrays):
    e = np.full(total, CANARY, dtype=np.uint8)
    for x, a in zip(offs, arrays):
        if a is not None:
            e[x:x + a.size] = a
    return e


def _same(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, int(bad[0]), int(bad.size))


# ------------------------------------------------------------------------------------------------ writes

def test_heap_writer_and_device_sink_write_the_image_of_grouped_sources(P, torch, made):
    m = made
    rc, dimage, dents, _ = _write(P, torch, m["names"], m["arrays"], m["mc"], m["elem"], "device")
    assert rc == OK and dimage == m["image"] and dents == m["ents"]
    # ... which is what zpack_amd_write_files_device writes from device buffers that already hold the grouped bytes
    for sink in ("heap", "device"):
        rc, gimage, gents, _ = _write(P, torch, m["names"], m["stored"], m["mc"], None, sink, call="plain")
        assert rc == OK and gimage == m["image"] and gents == m["ents"], sink
    # the noise of a float no longer sits between the bytes that compress: the grouped archive is the smaller one
    rc, pimage, _, _ = _write(P, torch, m["names"], m["arrays"], m["mc"], None, "heap", call="plain")
    assert rc == OK and len(m["image"]) < len(pimage)


def test_no_element_sizes_is_the_existing_call(P, torch, made):
    m = made
    names, arrays = m["names"][:14], m["arrays"][:14]
    rc, a, ea, _ = _write(P, torch, names, arrays, m["mc"], None, "heap", call="plain")
    for elem in (None, [1] * len(names)):
        for sink in ("heap", "device"):
            rc2, b, eb, _ = _write(P, torch, names, arrays, m["mc"], elem, sink)
            assert (rc2, b, eb) == (rc, a, ea) and rc == OK


def test_the_oracle_and_the_reference_read_grouped_bytes(made):
    m = made
    o = oracle()
    for (off, comp, unc, h, meth), want, name in zip(m["ents"], m["stored"], m["names"]):
        assert unc == want.size and meth == m["mc"][0]
        rc, out, got, hh = o.entry_decode(m["image"], off, comp, unc, h, meth, unc)
        assert rc == OK and out[:unc] == want.tobytes(), name
    if have_ref():
        z = ref()
        rc, r, keep = z.open_memory(m["image"])
        assert rc == OK and r.file_count == len(m["names"])
        try:
            for i, want in enumerate(m["stored"]):
                rc, out = z.read_file(r, i, want.size)
                assert rc == OK and out == want.tobytes(), m["names"][i]
        finally:
            z.close_reader(r)


@pytest.mark.parametrize("where", ["memory", "device"])
def test_test_files_says_ok_and_the_planes_read_returns_the_tensors(P, torch, made, where):
    m = made
    o = Opened(P, torch, m["image"], where)
    try:
        n = len(o.ents)
        res = (C.c_int * n)(*([-1] * n))
        assert P.lib.zpack_amd_test_files(C.byref(o.r), (PFE * n)(*[C.pointer(e) for e in o.ents]), n, res, None) == OK and list(res) == [OK] * n
        caps = [a.size for a in m["arrays"]]
        head, buf, offs = _read(P, torch, o, o.ents, caps, m["elem"])
        assert head == (OK, [OK] * n, 0)
        _same(buf, _want(buf.size, offs, m["arrays"]), "planes read")
        # the plain call returns the grouped bytes; the planes call without element sizes, or with ones, is the plain call
        headp, bufp, offs = _read(P, torch, o, o.ents, caps, None, call="plain")
        assert headp == head
        _same(bufp, _want(bufp.size, offs, m["stored"]), "plain read")
        for elem in (None, [1] * n):
            head1, buf1, _ = _read(P, torch, o, o.ents, caps, elem)
            assert head1 == head
            _same(buf1, bufp, "planes read without element sizes")
        # generous buffers, and a pick in another order: the bytes behind uncomp_size stay as they were
        pick = [n - 1, 3, 12, 0, 11, 13]
        ents = [o.ents[i] for i in pick]
        head2, buf2, offs2 = _read(P, torch, o, ents, [m["arrays"][i].size + 100 for i in pick], [m["elem"][i] for i in pick])
        assert head2 == (OK, [OK] * len(pick), 0)
        _same(buf2, _want(buf2.size, offs2, [m["arrays"][i] for i in pick]), "a pick with room to spare")
    finally:
        o.close()


# ------------------------------------------------------------------------------------------------ bad arguments, damaged entries

def test_an_element_size_of_three_is_stream_invalid_and_nothing_moves(P, torch, made):
    m = made
    names, arrays = m["names"][:6], m["arrays"][:6]
    for sink in ("heap", "device"):
        rc, image, ents, (at0, at1) = _write(P, torch, names, arrays, m["mc"], [2, 2, 3, 2, 4, 4], sink)      # (_write: the sources are as they were)
        assert rc == STREAM_INVALID and at1 == at0 and ents == []
    for where in ("memory", "device"):
        o = Opened(P, torch, m["image"], where)
        try:
            ents = o.ents[:4]
            head, buf, _ = _read(P, torch, o, ents, [int(e.uncomp_size) for e in ents], [2, 3, 2, 2])
            assert head[0] == STREAM_INVALID and head[1] == [-1] * 4 and bool((buf == CANARY).all())
        finally:
            o.close()


@pytest.mark.parametrize("where", ["memory", "device"])
def test_a_damaged_entry_has_the_plain_read_s_status_and_an_untouched_buffer(P, torch, made, where):
    m = made
    j = m["names"].index("fp32_4096")
    off, comp, unc, _, _ = m["ents"][j]
    cases = []
    broken = bytearray(m["image"]); broken[off] ^= 0xFF                                # the frame's first byte: no frame any more
    cases.append(("magic", bytes(broken), 0, True))
    broken = bytearray(m["image"]); broken[off + comp // 2] ^= 0xFF                    # somewhere inside: whatever the plain read says
    cases.append(("inside", bytes(broken), 0, False))
    cases.append(("comp_size", m["image"], 9, True))                                   # the entry's last bytes are not its own
    for what, image, cut, must_fail in cases:
        o = Opened(P, torch, image, where)
        try:
            mine = FileEntry.from_buffer_copy(o.ents[j])
            mine.comp_size -= cut
            ents = [o.ents[j - 1], mine, o.ents[j + 1]]
            idx = [j - 1, j, j + 1]
            caps = [m["arrays"][i].size for i in idx]
            elem = [m["elem"][i] for i in idx]
            headp, bufp, offs = _read(P, torch, o, ents, caps, None, call="plain")
            head, buf, offs = _read(P, torch, o, ents, caps, elem)
            assert head == headp, what                                                  # results, return value, last_return: the plain read's
            assert head[1][0] == OK and head[1][2] == OK
            st = head[1][1]
            if must_fail:
                assert st not in (OK, HASH_MISMATCH), (what, st)
            delivered = bufp[offs[1]:offs[1] + unc]
            if st == OK or (st == HASH_MISMATCH and not bool((delivered[-8:] == CANARY).all())):
                # (decoded to all of its bytes, right or wrong — the plain read wrote the entry's last bytes —: the join of what that delivers)
                middle = np.empty(unc, dtype=np.uint8)
                mm = unc // elem[1]
                middle[:mm * elem[1]] = delivered[:mm * elem[1]].reshape(elem[1], mm).T.reshape(-1)
            else:
                middle = None                                                           # untouched between its canaries
            _same(buf, _want(buf.size, offs, [m["arrays"][j - 1], middle, m["arrays"][j + 1]]), what)
        finally:
            o.close()


# ------------------------------------------------------------------------------------------------ the codec's counts

def test_planes_stats_count_rows_launches_and_staged_entries(torch, made):
    m = made
    n = len(m["names"])
    grouped_rows = sum(1 for a, k in zip(m["arrays"], m["elem"]) if k > 1 and a.size)
    assert grouped_rows == 14                                                           # 12 tensors, the tail, the 3 MiB entry; not the empty one, not the bytes
    codec = zpack_amd.Codec(0)
    try:
        # ---- writing into a sink ----
        buf, addr, _ = _on_device(torch, m["arrays"])
        desc = np.zeros(n, dtype=zpack_amd.ENCODE_DESC)
        desc["size"] = [a.size for a in m["arrays"]]
        desc["method"], desc["level"] = m["mc"]
        desc["dst_capacity"] = [codec.compress_bound(m["mc"][0], a.size) for a in m["arrays"]]
        sink = torch.empty(int(desc["dst_capacity"].sum()) + 64, dtype=torch.uint8, device="cuda:0")
        res1, placed, nbytes1 = codec.encode_batch_dsink(addr, desc, sink, src_on_device=True, elem=[1] * n)
        assert placed == n and codec.planes_stats() == dict(split=0, joined=0, launches=0, staged=0)
        plain_sink = sink[:nbytes1].cpu().numpy().copy()
        res0, placed, nbytes0 = codec.encode_batch_dsink(addr, desc, sink, src_on_device=True)
        assert placed == n and nbytes0 == nbytes1 and np.array_equal(res0, res1) and np.array_equal(sink[:nbytes0].cpu().numpy(), plain_sink)
        res2, placed, nbytes2 = codec.encode_batch_dsink(addr, desc, sink, src_on_device=True, elem=m["elem"])
        assert placed == n and codec.planes_stats() == dict(split=grouped_rows, joined=0, launches=1, staged=0)
        assert [int(h) for h in res2["hash"]] == [e[3] for e in m["ents"]] and nbytes2 == sum(e[1] for e in m["ents"])
        # ---- reading: the image in host memory, then in device memory ----
        dd = np.zeros(n, dtype=zpack_amd.DECODE_DESC)
        for i, (off, comp, unc, h, meth) in enumerate(m["ents"]):
            dd[i] = (off, comp, unc, h, 0, unc, meth, 0)
        offs, total = _layout([a.size for a in m["arrays"]], MIS)
        out = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda:0")
        ptrs = [out.data_ptr() + x for x in offs]
        want = _want(total, offs, m["arrays"])
        arc = np.frombuffer(m["image"], dtype=np.uint8)
        res = codec.decode_batch_host_dptr(arc, dd, ptrs, elem=[1] * n)
        assert (res["status"] == OK).all() and codec.planes_stats() == dict(split=0, joined=0, launches=0, staged=0)
        out.fill_(CANARY)
        res = codec.decode_batch_host_dptr(arc, dd, ptrs, elem=m["elem"])
        torch.cuda.synchronize()
        st = codec.planes_stats()
        assert (res["status"] == OK).all() and st["split"] == 0 and st["joined"] == grouped_rows
        assert st["staged"] >= 1 and st["launches"] == st["staged"] + 1                 # the 3 MiB frame (at least) block-parallel through the staging; one launch for the rest
        _same(out.cpu().numpy(), want, "host image")
        image_t = torch.from_numpy(arc.copy()).to("cuda:0")
        out.fill_(CANARY)
        res = codec.decode_batch_dimage(image_t, dd, ptrs, elem=m["elem"])
        torch.cuda.synchronize()
        assert (res["status"] == OK).all() and codec.planes_stats() == dict(split=0, joined=grouped_rows, launches=1, staged=0)
        _same(out.cpu().numpy(), want, "device image")
        # host destinations take no element size but 1
        L = zpack_amd.lib()
        L.zpk_codec_decode_batch_dimage_planes.argtypes = [C.c_void_p] * 2 + [C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        hres = np.zeros(n, dtype=zpack_amd.DECODE_RESULT)
        houts = [np.zeros(max(a.size, 1), dtype=np.uint8) for a in m["arrays"]]
        hp = (C.c_void_p * n)(*[h.ctypes.data for h in houts])
        assert L.zpk_codec_decode_batch_dimage_planes(codec.h, image_t.data_ptr(), image_t.numel(), dd.ctypes.data, n, hp, 0, hres.ctypes.data, (C.c_uint8 * n)(*m["elem"])) == -2
    finally:
        codec.close()


def test_the_pipeline_joins_piece_by_piece(torch):
    """12 288 x 16 KiB LZ4 entries, large enough for the host path's three-stage pipeline: 128 written (fp32 as planes of 4, every fourth
    one as plain bytes), their payloads repeated 96 times in the image; every piece's slots are joined behind its decode"""
    from tests import zpk
    g = torch.Generator().manual_seed(12288)
    src = (torch.randn(128, 4096, generator=g) * 0.02).to("cuda:0")
    tensors = {"t%03d" % i: src[i] for i in range(128)}
    elem128 = [1 if i % 4 == 3 else 4 for i in range(128)]
    arc = device_io.write_files_device(None, tensors, method=METHOD_LZ4, level=0, planes={n: k for n, k in zip(tensors, elem128)})
    ents = zpk.parse(arc)
    lo, hi = ents[0]["offset"], ents[-1]["offset"] + ents[-1]["comp_size"]
    region = np.frombuffer(arc, dtype=np.uint8)[lo:hi]
    reps, n = 96, 96 * 128
    image = np.concatenate([np.zeros(10, dtype=np.uint8), np.tile(region, reps), np.zeros(64, dtype=np.uint8)])
    desc = np.zeros(n, dtype=zpack_amd.DECODE_DESC)
    rel = np.array([e["offset"] - lo for e in ents], dtype=np.uint64)
    desc["src_offset"] = np.uint64(10) + np.repeat(np.arange(reps, dtype=np.uint64) * np.uint64(hi - lo), 128) + np.tile(rel, reps)
    desc["comp_size"] = np.tile(np.array([e["comp_size"] for e in ents], dtype=np.uint64), reps)
    desc["expect_hash"] = np.tile(np.array([e["hash"] for e in ents], dtype=np.uint64), reps)
    desc["uncomp_size"] = desc["dst_capacity"] = 16384
    desc["method"] = METHOD_LZ4
    out = torch.full((n * 16384 + 2 * GAP,), CANARY, dtype=torch.uint8, device="cuda:0")
    ptrs = [out.data_ptr() + GAP + i * 16384 for i in range(n)]
    codec = zpack_amd.Codec(0)
    try:
        res = codec.decode_batch_host_dptr(image, desc, ptrs, elem=elem128 * reps)
        torch.cuda.synchronize()
        st, ps = codec.decode_stats(), codec.planes_stats()
        assert st["pipelined_sub_batches"] >= 1, st
        assert (res["status"] == OK).all() and (res["produced"] == 16384).all()
        assert ps["joined"] == 96 * 96 and ps["split"] == 0 and ps["staged"] == 0 and ps["launches"] >= 3, ps      # one launch per piece
        assert st["span_copy_launches"] == ps["launches"]                               # ... beside the k_span_copy of its plain entries
        want = src.view(torch.uint8).reshape(-1).repeat(reps)
        assert torch.equal(out[GAP:GAP + n * 16384], want)
        assert bool((out[:GAP] == CANARY).all()) and bool((out[GAP + n * 16384:] == CANARY).all())
    finally:
        codec.close()


def test_large_stored_entries_are_joined_from_their_group(torch):
    """stored entries past 512 KiB are read in pieces as one group of the host path: its slots are joined by one launch"""
    from tests import zpk
    g = torch.Generator().manual_seed(77)
    tensors = {"a.fp64": (torch.randn((1 << 17) + 1, generator=g, dtype=torch.float64) * 0.02).to("cuda:0"),
               "b.bf16": (torch.randn(300 * 1024 + 3, generator=g) * 0.02).to(torch.bfloat16).to("cuda:0"),
               "c.u8": (torch.arange(700000, device="cuda:0") % 251).to(torch.uint8),
               "d.fp32": (torch.randn(100, generator=g) * 0.02).to("cuda:0")}
    elem = {"a.fp64": 8, "b.bf16": 2, "c.u8": 1, "d.fp32": 4}
    raw = {k: t.view(-1).view(torch.uint8).cpu().numpy() for k, t in tensors.items()}
    arc = device_io.write_files_device(None, tensors, method=0, level=0, planes=elem)
    ents = zpk.parse(arc)
    for e in ents:                                                                      # stored: the payload IS the grouped bytes
        assert e["comp_size"] == e["uncomp_size"] and arc[e["offset"]:e["offset"] + e["comp_size"]] == grouped(raw[e["filename"]], elem[e["filename"]]).tobytes()
    outs, status = device_io.read_files_device(arc, planes=elem)
    assert status == [OK] * 4 and all(np.array_equal(o.cpu().numpy(), raw[k]) for o, k in zip(outs, tensors))
    desc = np.zeros(4, dtype=zpack_amd.DECODE_DESC)
    for i, e in enumerate(ents):
        desc[i] = (e["offset"], e["comp_size"], e["uncomp_size"], e["hash"], 0, e["uncomp_size"], 0, 0)
    offs, total = _layout([e["uncomp_size"] for e in ents], MIS)
    out = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda:0")
    codec = zpack_amd.Codec(0)
    try:
        res = codec.decode_batch_host_dptr(np.frombuffer(arc, dtype=np.uint8), desc, [out.data_ptr() + x for x in offs], elem=[elem[e["filename"]] for e in ents])
        torch.cuda.synchronize()
        assert (res["status"] == OK).all() and codec.decode_stats()["frame_parallel_entries"] == 3        # a, b, c in pieces; d with the rest
        assert codec.planes_stats() == dict(split=0, joined=3, launches=2, staged=0)    # the group's two grouped entries in one launch, d in the rest's
        _same(out.cpu().numpy(), _want(total, offs, [raw[e["filename"]] for e in ents]), "stored group")
    finally:
        codec.close()


# ------------------------------------------------------------------------------------------------ the torch view

@pytest.mark.parametrize("mc", METHODS)
def test_device_io_round_trip_with_dtype_planes_and_the_manifest(torch, mc):
    g = torch.Generator().manual_seed(5)
    tensors = {
        "w.bf16": (torch.randn(300, 70, generator=g) * 0.02).to(torch.bfloat16).to("cuda:0"),
        "w.fp16": (torch.randn(4097, generator=g) * 0.02).to(torch.float16).to("cuda:0"),
        "w.fp32": (torch.randn(65537, generator=g) * 0.02).to("cuda:0"),
        "w.fp64": (torch.randn(513, generator=g, dtype=torch.float64) * 0.02).to("cuda:0"),
        "ids.int64": torch.arange(1000, dtype=torch.int64, device="cuda:0"),
        "mask.u8": (torch.arange(777, device="cuda:0") % 3).to(torch.uint8),
        "none": torch.zeros(0, dtype=torch.float32, device="cuda:0"),
    }
    want_elem = {"w.bf16": 2, "w.fp16": 2, "w.fp32": 4, "w.fp64": 8, "ids.int64": 1, "mask.u8": 1, "none": 4}
    raw = {k: t.contiguous().view(-1).view(torch.uint8).cpu().numpy() for k, t in tensors.items()}
    image = device_io.write_archive_device(tensors, method=mc[0], level=mc[1], planes="dtype")
    assert image.is_cuda and device_io.write_files_device(None, tensors, method=mc[0], level=mc[1], planes="dtype") == image.cpu().numpy().tobytes()
    # read back through the manifest: the tensors' bytes, the manifest entry not among them
    outs, status = device_io.read_files_device(image, planes="manifest")
    assert status == [OK] * len(tensors) and len(outs) == len(tensors)
    for (name, t), got in zip(tensors.items(), outs):
        assert np.array_equal(got.cpu().numpy(), raw[name]), name
        assert torch.equal(got.view(t.dtype).reshape(t.shape), t) if t.numel() else got.numel() == 0
    outs, status = device_io.read_files_device(image, names=["w.fp32", "mask.u8"], planes="manifest")
    assert status == [OK, OK] and np.array_equal(outs[0].cpu().numpy(), raw["w.fp32"]) and np.array_equal(outs[1].cpu().numpy(), raw["mask.u8"])
    outs, status = device_io.read_files_device(image.cpu().numpy().tobytes(), planes=want_elem)            # (a memory reader, the map handed in)
    assert status == [OK] * (len(tensors) + 1)
    for name, got in zip(tensors, outs):
        assert np.array_equal(got.cpu().numpy(), raw[name]), name
    # without planes the same image is an ordinary archive: the manifest is an entry, the tensors' entries hold grouped bytes
    outs, status = device_io.read_files_device(image)
    assert status == [OK] * (len(tensors) + 1) and device_io.test_files(image) == [OK] * (len(tensors) + 1)
    import json
    assert json.loads(outs[-1].cpu().numpy().tobytes().decode()) == want_elem
    for name, got in zip(tensors, outs):
        assert np.array_equal(got.cpu().numpy(), grouped(raw[name], want_elem[name])), name
    # planes=None writes what it always wrote; a dict names the entries; an archive without a manifest raises
    plain_image = device_io.write_archive_device(tensors, method=mc[0], level=mc[1])
    assert plain_image.numel() > image.numel()
    by_dict = device_io.write_archive_device(tensors, method=mc[0], level=mc[1], planes={"w.fp32": 4})
    outs, status = device_io.read_files_device(by_dict, planes={"w.fp32": 4})
    assert status == [OK] * len(tensors) and all(np.array_equal(got.cpu().numpy(), raw[name]) for name, got in zip(tensors, outs))
    with pytest.raises(KeyError):
        device_io.read_files_device(plain_image, planes="manifest")
    with pytest.raises(RuntimeError):
        device_io.write_archive_device(tensors, method=mc[0], level=mc[1], planes={"w.fp32": 3})
