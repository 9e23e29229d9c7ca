"""GPU: a reader over an archive image in DEVICE memory (include/zpack_amd.h: zpack_amd_init_reader_device), every read call on it, and the
codec call behind the batch reads (zpk_codec_decode_batch_dimage: sub-batches through the codec's staging, dimage_plan.h).

The reference of every read is the same call of the same library on a MEMORY reader over the same bytes: the same return value, the
same results, the same last_return, and the same bytes in all of [buffer, buffer + max_size) — host and device buffers start out as
0xA5, so a byte the memory reader's call does not write must not be written here either — with 64 canary bytes around every
destination intact.  Memory comes from torch."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import zpack_amd
from benchdata import datagen as dg
from tests import zpk
from tests._libs import Reader, Writer, FileEntry, Stream, u8p, METHOD_NONE, METHOD_ZSTD, METHOD_LZ4
from tests.device_mem import torch, Z, _plain, _build, _layout, CANARY, GAP            # noqa: F401  (torch, Z: fixtures)

pytestmark = pytest.mark.gpu

PFE = C.POINTER(FileEntry)
NOT_LOADED, FILE_TOO_SMALL, STREAM_INVALID, NOT_AVAILABLE = 1, 5, 21, 24


# ------------------------------------------------------------------------------------------------ helpers

def _image(torch, arc, shift=0):
    """the archive's bytes in device memory, `shift` bytes into their allocation -> (the tensor, the image's address)"""
    t = torch.full((shift + len(arc) + 3,), 0xEE, dtype=torch.uint8, device="cuda:0")
    t[shift:shift + len(arc)] = torch.from_numpy(np.frombuffer(arc, dtype=np.uint8).copy())
    torch.cuda.synchronize()
    return t, t.data_ptr() + shift


def _open_dev(Z, torch, arc, shift=0):
    t, at = _image(torch, arc, shift)
    r = Reader()
    rc = Z.lib.zpack_amd_init_reader_device(C.byref(r), at, len(arc))
    assert rc == 0, rc
    return r, t


def _open_mem(Z, arc):
    keep = (C.c_uint8 * len(arc)).from_buffer_copy(arc)
    r = Reader()
    assert Z.lib.zpack_init_reader_memory_shared(C.byref(r), C.cast(keep, u8p), len(arc)) == 0
    return r, keep


def _ents(r, picks):
    """picks: indices into the reader's own table, or FileEntry objects (copies with changed fields)"""
    return [r.file_entries[p] if isinstance(p, (int, np.integer)) else p for p in picks]


def _buffer(torch, total, where):
    if where == "host":
        buf = np.full(total, CANARY, dtype=np.uint8)
        return buf, buf.ctypes.data
    buf = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    return buf, buf.data_ptr()


def _host_copy(torch, buf):
    if isinstance(buf, np.ndarray):
        return buf
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def _read(Z, torch, r, picks, caps, where, mis=(0,), dctx=None):
    """zpack_read_files (where = "host") / zpack_amd_read_files_device ("device") into destinations laid out by _layout
    -> (rc, results, last_return), the whole buffer, the destinations' offsets"""
    ents = _ents(r, picks)
    n = len(ents)
    offs, total = _layout(caps, mis)
    buf, base = _buffer(torch, total, where)
    res = (C.c_int * max(n, 1))(*([-1] * max(n, 1)))
    fn = Z.lib.zpack_read_files if where == "host" else Z.lib.zpack_amd_read_files_device
    rc = fn(C.byref(r), (PFE * max(n, 1))(*[C.pointer(e) for e in ents]), n, (C.c_void_p * max(n, 1))(*[base + o for o in offs]),
            (C.c_size_t * max(n, 1))(*caps), res, dctx)
    return (rc, list(res)[:n], int(r.last_return)), _host_copy(torch, buf), offs


def _read_packed(Z, torch, r, picks, size, where):
    ents = _ents(r, picks)
    n = len(ents)
    buf, base = _buffer(torch, GAP + size + GAP, where)
    offs = (C.c_uint64 * n)()
    res = (C.c_int * n)(*([-1] * n))
    fn = Z.lib.zpack_read_files_packed if where == "host" else Z.lib.zpack_amd_read_files_device_packed
    rc = fn(C.byref(r), (PFE * n)(*[C.pointer(e) for e in ents]), n, base + GAP, size, offs, res, None)
    return (rc, list(res), int(r.last_return), list(offs)), _host_copy(torch, buf)


def _same_bytes(got, want, offs, caps, results, bytes_of=(0, 15)):
    """the whole buffers are equal, canaries included; the bytes of an entry whose verdict is not one of bytes_of are the decoder's
    leftovers (the verdict is the contract there) and are left out"""
    got = got.copy()
    for o, c, v in zip(offs, caps, results):
        if v not in bytes_of:
            got[o:o + c] = want[o:o + c]
    if not np.array_equal(got, want):
        bad = int(np.flatnonzero(got != want)[0])
        raise AssertionError("byte %d of the buffer differs: %d, want %d (destinations at %s...)" % (bad, got[bad], want[bad], offs[:4]))


def _same_as_memory(Z, torch, rm, rd, picks_m, picks_d, caps, mis=(0,), want=None):
    """host and device destinations: the device reader's call against the memory reader's (want: its results, computed before)"""
    out = {}
    for where in ("host", "device"):
        ref = want[where] if want else _read(Z, torch, rm, picks_m, caps, where, mis)
        got = _read(Z, torch, rd, picks_d, caps, where, mis)
        assert got[0] == ref[0], (where, got[0], ref[0])
        assert got[2] == ref[2]
        _same_bytes(got[1], ref[1], ref[2], caps, ref[0][1])
        out[where] = ref
    return out


def _desc_of(arc, caps=None):
    pe = zpk.parse(arc)
    desc = np.zeros(len(pe), dtype=zpack_amd.DECODE_DESC)
    for k, (d, e) in enumerate(zip(desc, pe)):
        d["src_offset"], d["comp_size"], d["uncomp_size"], d["expect_hash"] = e["offset"], e["comp_size"], e["uncomp_size"], e["hash"]
        d["dst_capacity"], d["method"] = (caps[k] if caps else e["uncomp_size"]), e["method"]
    return desc


# ------------------------------------------------------------------------------------------------ the shared archive and its reference

@pytest.fixture(scope="module")
def mixed():
    """~200 entries in the three methods: the sizes around 64 KiB, 0 and 1, a few up to 300 KiB, the rest under 6000 bytes"""
    sizes = [0, 1, 65535, 65536, 65537] * 3 + [300 << 10, 200 * 1024 + 3, 131072 + 1, 100000]
    rng = np.random.default_rng(17)
    sizes += [int(x) for x in rng.integers(2, 6000, 201 - len(sizes))]
    methods = [(dg.NONE, 0), (dg.LZ4, 0), (dg.ZSTD, 3)]
    specs = []
    for i, n in enumerate(sizes):
        m, lv = methods[(i % 5 + i // 5) % 3]                                          # every edge size in every method
        specs.append((m, lv, _plain(i, n)))
    arc = _build(specs)
    order = [int(x) for x in np.random.default_rng(19).permutation(len(specs))]
    if specs[order[-1]][2] == b"":                                                     # (the packed forms want bytes in their last entry)
        order.append(next(i for i in order if len(specs[i][2]) > 1000))
    caps = [len(specs[i][2]) + (7 if k % 4 == 1 else 0) for k, i in enumerate(order)]  # some with room to spare
    return dict(arc=arc, plains=[s[2] for s in specs], order=order, caps=caps)


@pytest.fixture(scope="module")
def mixed_ref(Z, torch, mixed):
    """what the MEMORY reader gives for the shuffled batch in the four forms: computed once, compared against and never changed"""
    rm, keep = _open_mem(Z, mixed["arc"])
    try:
        ref = {w: _read(Z, torch, rm, mixed["order"], mixed["caps"], w, (1, 7, 15)) for w in ("host", "device")}
        pos = 0
        for i in mixed["order"][:-1]:
            pos += (len(mixed["plains"][i]) + 255) & ~255
        size_dev = pos + len(mixed["plains"][mixed["order"][-1]]) - 1                  # one byte short for the last entry
        size_host = sum(len(mixed["plains"][i]) for i in mixed["order"]) - 1
        ref["packed_host"] = (size_host,) + _read_packed(Z, torch, rm, mixed["order"], size_host, "host")
        ref["packed_device"] = (size_dev,) + _read_packed(Z, torch, rm, mixed["order"], size_dev, "device")
        assert ref["host"][0][:2] == (0, [0] * len(mixed["order"])) and ref["device"][0] == ref["host"][0]
        assert ref["packed_host"][1][1] == [0] * (len(mixed["order"]) - 1) + [12] and ref["packed_device"][1][1] == ref["packed_host"][1][1]
        return ref
    finally:
        Z.lib.zpack_close_reader(C.byref(rm))


# ------------------------------------------------------------------------------------------------ 1. the golden archives

@pytest.mark.parametrize("name", ["archive_none.zpk", "archive_zstd.zpk", "archive_lz4.zpk"])
def test_golden_archives_read_like_a_memory_reader(Z, torch, golden_dir, name):
    arc = open(os.path.join(golden_dir, "ref_workdir", name), "rb").read()
    rm, keep = _open_mem(Z, arc)
    rd, image = _open_dev(Z, torch, arc)
    try:
        for f in ("version", "file_count", "comp_size", "uncomp_size", "file_size", "cdr_offset", "eocdr_offset"):
            assert getattr(rd, f) == getattr(rm, f), f
        assert rd.file_count == 2 and not rd.buffer and not rd.file
        for i in range(rd.file_count):
            for f in ("filename", "offset", "comp_size", "uncomp_size", "hash", "comp_method"):
                assert getattr(rd.file_entries[i], f) == getattr(rm.file_entries[i], f), (i, f)
        p, dev = C.c_void_p(), C.c_int(-5)
        assert Z.lib.zpack_amd_reader_device_image(C.byref(rd), C.byref(p), C.byref(dev)) == 0 and (p.value, dev.value) == (image.data_ptr(), 0)
        assert Z.lib.zpack_amd_reader_device_image(C.byref(rm), C.byref(p), C.byref(dev)) == 0 and (p.value, dev.value) == (None, -1)
        assert Z.lib.zpack_read_archive_memory(C.byref(rd)) == NOT_LOADED and Z.lib.zpack_read_archive(C.byref(rd)) == NOT_LOADED     # no host image, no file
        plains = [open(os.path.join(golden_dir, "ref_workdir", n), "rb").read() for n in ("file1.txt", "file2.txt")]
        assert [len(x) for x in plains] == [169, 349]
        # zpack_read_files, zpack_amd_read_files_device
        ref = _same_as_memory(Z, torch, rm, rd, [0, 1], [0, 1], [350, 350], mis=(0, 5))
        for where in ("host", "device"):
            (rc, res, last), buf, offs = ref[where]
            assert (rc, res) == (0, [0, 0])
            (rc, res, last), buf, offs = _read(Z, torch, rd, [0, 1], [350, 350], where, (0, 5))
            assert [buf[o:o + len(x)].tobytes() for o, x in zip(offs, plains)] == plains
        # the packed forms
        for where, size in (("host", 169 + 349), ("device", 256 + 349)):
            want, wbuf = _read_packed(Z, torch, rm, [0, 1], size, where)
            got, gbuf = _read_packed(Z, torch, rd, [0, 1], size, where)
            assert got == want and want[:2] == (0, [0, 0]) and np.array_equal(gbuf, wbuf)
            assert gbuf[GAP + want[3][1]:GAP + want[3][1] + 349].tobytes() == plains[1]
        # zpack_read_file
        for i in (0, 1):
            outs = []
            for r in (rm, rd):
                out = np.full(GAP + 350 + GAP, CANARY, dtype=np.uint8)
                rc = Z.lib.zpack_read_file(C.byref(r), C.pointer(r.file_entries[i]), out.ctypes.data + GAP, 350, None)
                outs.append((rc, int(r.last_return), out.tobytes()))
            assert outs[0] == outs[1] and outs[0][0] == 0 and outs[1][2][GAP:GAP + len(plains[i])] == plains[i]
    finally:
        Z.lib.zpack_close_reader(C.byref(rd))
        Z.lib.zpack_close_reader(C.byref(rm))


# ------------------------------------------------------------------------------------------------ 2. the mixed archive

@pytest.mark.parametrize("shift", [0, 1, 7])
def test_mixed_archive_shuffled_misaligned_and_packed(Z, torch, mixed, mixed_ref, shift):
    rd, image = _open_dev(Z, torch, mixed["arc"], shift)
    try:
        order, caps = mixed["order"], mixed["caps"]
        _same_as_memory(Z, torch, None, rd, None, order, caps, mis=(1, 7, 15), want=mixed_ref)
        (rc, res, last), buf, offs = _read(Z, torch, rd, order, caps, "device", (1, 7, 15))
        for i, o in zip(order, offs):
            assert buf[o:o + len(mixed["plains"][i])].tobytes() == mixed["plains"][i], i
        for where in ("host", "device"):
            size, want, wbuf = mixed_ref["packed_" + where]
            got, gbuf = _read_packed(Z, torch, rd, order, size, where)
            assert got == want, where
            assert np.array_equal(gbuf, wbuf), (where, int(np.flatnonzero(gbuf != wbuf)[0]))
        assert image[:shift].cpu().tolist() == [0xEE] * shift and image[shift + len(mixed["arc"]):].cpu().tolist() == [0xEE] * 3
        assert image[shift:shift + len(mixed["arc"])].cpu().numpy().tobytes() == mixed["arc"]         # the image is read-only to the library
    finally:
        Z.lib.zpack_close_reader(C.byref(rd))


# ------------------------------------------------------------------------------------------------ 3. verdicts beside good entries

def test_verdicts_in_one_batch_with_good_entries(Z, torch, mixed):
    arc = mixed["arc"]
    ents0 = zpk.parse(arc)
    pick = {}                                                                          # per method: entries of a few KiB to change
    for i, e in enumerate(ents0):
        if 3000 < e["uncomp_size"] < 6000 and e["comp_size"] > 200:
            pick.setdefault(e["method"], []).append(i)
    assert all(len(pick[m]) >= 4 for m in (0, 1, 2))
    flip_lz4, flip_zstd = pick[METHOD_LZ4][0], pick[METHOD_ZSTD][0]
    damaged = bytearray(arc)
    for i in (flip_lz4, flip_zstd):
        damaged[ents0[i]["offset"] + ents0[i]["comp_size"] // 2] ^= 0x40               # one flipped payload byte
    damaged = bytes(damaged)
    changed = {"wrong_hash": pick[METHOD_LZ4][1], "too_large": pick[METHOD_ZSTD][1], "too_small": pick[METHOD_LZ4][2], "at_end": pick[METHOD_NONE][0],
               "method7": pick[METHOD_ZSTD][2], "one_short": pick[METHOD_LZ4][3], "empty": pick[METHOD_NONE][1], "too_large_stored": pick[METHOD_NONE][2]}
    good = [i for i in range(60) if i not in changed.values() and i not in (flip_lz4, flip_zstd)][:20]
    rm, keep = _open_mem(Z, damaged)
    rd, image = _open_dev(Z, torch, damaged, 1)
    try:
        batch = good[:10] + [flip_lz4, flip_zstd] + list(changed.values()) + good[10:]
        names = {v: k for k, v in changed.items()}
        picks, caps = {id(rm): [], id(rd): []}, []
        for i in batch:
            cap = None
            for r in (rm, rd):
                e = FileEntry.from_buffer_copy(r.file_entries[i])
                what = names.get(i)
                if what == "wrong_hash":
                    e.hash ^= 1
                elif what in ("too_large", "too_large_stored"):
                    e.uncomp_size += 1
                elif what == "too_small":
                    e.uncomp_size -= 1
                elif what == "at_end":
                    e.offset = len(arc) - e.comp_size                                  # offset + comp_size == file_size
                elif what == "method7":
                    e.comp_method = 7
                elif what == "empty":
                    e.comp_size = 0
                cap = int(e.uncomp_size) - (1 if what == "one_short" else 0)
                picks[id(r)].append(e)
            caps.append(cap)
        ref = _same_as_memory(Z, torch, rm, rd, picks[id(rm)], picks[id(rd)], caps, mis=(0, 9))
        assert ref["device"][0] == ref["host"][0]
        by = dict(zip(batch, ref["host"][0][1]))
        assert by[changed["wrong_hash"]] == 15 and by[changed["at_end"]] == 16 and by[changed["one_short"]] == 12 and by[changed["empty"]] == 0
        assert all(by[changed[k]] != 0 for k in ("method7", "too_large", "too_large_stored", "too_small")) and by[flip_lz4] != 0 and by[flip_zstd] != 0      # (whatever the memory reader says: compared above)
        assert all(by[i] == 0 for i in good)
    finally:
        Z.lib.zpack_close_reader(C.byref(rd))
        Z.lib.zpack_close_reader(C.byref(rm))


# ------------------------------------------------------------------------------------------------ 4. the large routes; 7. raw, streamed and copied reads

@pytest.fixture(scope="module")
def large():
    n = (1 << 20) + 5
    specs = [(dg.LZ4, 0, _plain(0, n)), (dg.ZSTD, 3, _plain(3, n)), (dg.NONE, 0, _plain(1, 2 << 20)), (dg.LZ4, 0, _plain(6, 5000))]
    return _build(specs), [s[2] for s in specs]


def test_large_entries_take_the_device_routes(Z, torch, large):
    arc, plains = large
    rm, keep = _open_mem(Z, arc)
    rd, image = _open_dev(Z, torch, arc, 7)
    try:
        caps = [len(x) for x in plains]
        ref = _same_as_memory(Z, torch, rm, rd, [0, 1, 2, 3], [0, 1, 2, 3], caps, mis=(3, 0, 11))
        for where in ("host", "device"):
            (rc, res, last), buf, offs = ref[where]
            assert (rc, res) == (0, [0, 0, 0, 0])
            assert [buf[o:o + len(x)].tobytes() for o, x in zip(offs, plains)] == plains
    finally:
        Z.lib.zpack_close_reader(C.byref(rd))
        Z.lib.zpack_close_reader(C.byref(rm))
    # the codec call itself says which routes the entries took
    codec = zpack_amd.Codec(0)
    t, at = _image(torch, arc)
    desc = _desc_of(arc)
    offs, total = _layout([int(x) for x in desc["dst_capacity"]], (3, 0, 11))
    buf = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda:0")
    dres = codec.decode_batch_dimage(t[:len(arc)], desc, [buf.data_ptr() + o for o in offs])
    st, ds = codec.decode_stats(), codec.dimage_stats()
    print("routes: walked %d, accepted %d, stored spans %d; dimage %s" % (st["device_walked"], st["device_walk_accepted"], st["stored_span_entries"], ds))
    assert (dres["status"] == 0).all() and [int(x) for x in dres["produced"]] == [len(x) for x in plains]
    assert st["device_walked"] >= 2 and st["device_walk_accepted"] >= 2 and st["stored_span_entries"] >= 1
    assert ds == dict(sub_batches=1, span_copy_launches=1, bytes_copied_home=0)
    got = _host_copy(torch, buf)
    want = np.full(total, CANARY, dtype=np.uint8)
    for o, x in zip(offs, plains):
        want[o:o + len(x)] = np.frombuffer(x, dtype=np.uint8)
    assert np.array_equal(got, want)
    hres, houts = codec.decode_batch_dimage(t[:len(arc)], desc)                       # host destinations
    assert hres.tobytes() == dres.tobytes() and [o.tobytes() for o in houts] == plains
    assert codec.dimage_stats()["bytes_copied_home"] > 0 and codec.dimage_stats()["span_copy_launches"] == 0
    # the pointer checks of the call: an archive range that leaves its allocation, a host destination -> ZPK_E_INVALID, nothing has run
    buf.fill_(CANARY); torch.cuda.synchronize()
    host = np.full(1 << 21, CANARY, dtype=np.uint8)
    L = zpack_amd.lib()
    res = np.zeros(len(desc), dtype=zpack_amd.DECODE_RESULT)
    good = [buf.data_ptr() + o for o in offs]
    for image_at, image_size, ptrs in ((t.data_ptr(), 1 << 40, good), (host.ctypes.data, len(arc), good), (t.data_ptr(), len(arc), good[:2] + [host.ctypes.data] + good[3:])):
        rc = L.zpk_codec_decode_batch_dimage(codec.h, image_at, image_size, desc.ctypes.data, len(desc), (C.c_void_p * 4)(*ptrs), 1, res.ctypes.data)
        assert rc == -2
    torch.cuda.synchronize()
    assert bool((buf == CANARY).all()) and bool((host == CANARY).all()) and not res.tobytes().strip(b"\0")
    codec.close()


def _stream(Z, r, i, in_window, out_window):
    """zpack_read_file_stream with the caller's loop of the reference's read_archive.c -> (rc, the bytes)"""
    st = Stream()
    assert Z.lib.zpack_init_stream(C.byref(st)) == 0
    in_buf, out_buf = (C.c_uint8 * in_window)(), (C.c_uint8 * out_window)()
    e = r.file_entries[i]
    out, rc = bytearray(), 0
    Z.lib.zpack_reset_stream(C.byref(st))
    for _ in range(1_000_000):
        if st.read_back:
            C.memmove(in_buf, C.string_at(C.addressof(st.next_in.contents) - st.read_back, st.read_back), st.read_back)
        st.next_in = C.cast(in_buf, u8p); st.avail_in = in_window
        st.next_out = C.cast(out_buf, u8p); st.avail_out = out_window
        rc = Z.lib.zpack_read_file_stream(C.byref(r), C.byref(e), C.byref(st), None)
        out += bytes(out_buf[:out_window - st.avail_out])
        if rc != 0 or (st.total_in == e.comp_size and st.total_out == e.uncomp_size and st.read_back == 0):
            break
    Z.lib.zpack_close_stream(C.byref(st))
    return rc, bytes(out)


def test_raw_streamed_and_copied_reads(Z, torch, golden_dir, large):
    arc, plains = large
    gold = open(os.path.join(golden_dir, "ref_workdir", "archive_zstd.zpk"), "rb").read()
    rm, keep = _open_mem(Z, arc)
    rd, image = _open_dev(Z, torch, arc, 1)
    gm, gkeep = _open_mem(Z, gold)
    gd, gimage = _open_dev(Z, torch, gold)
    try:
        pe = zpk.parse(arc)
        for i, cap in ((0, pe[0]["comp_size"]), (3, pe[3]["comp_size"] + 9), (2, 1000), (3, 0)):
            outs = []
            for r in (rm, rd):
                out = np.full(GAP + cap + GAP, CANARY, dtype=np.uint8)
                outs.append((Z.lib.zpack_read_raw_file(C.byref(r), C.pointer(r.file_entries[i]), out.ctypes.data + GAP, cap), out.tobytes()))
            assert outs[0] == outs[1] and outs[0][0] == 0
            n = min(cap, pe[i]["comp_size"])
            assert outs[1][1][GAP:GAP + n] == arc[pe[i]["offset"]:pe[i]["offset"] + n]
        past = FileEntry.from_buffer_copy(rd.file_entries[0])
        past.offset = len(arc) - 5
        assert Z.lib.zpack_read_raw_file(C.byref(rd), C.pointer(past), keep, 16) == Z.lib.zpack_read_raw_file(C.byref(rm), C.pointer(past), keep, 16) == 16
        # streamed: a 16-byte input window on a golden entry, a 128 KiB window on the 1 MiB LZ4 entry
        want = open(os.path.join(golden_dir, "ref_workdir", "file2.txt"), "rb").read()
        assert _stream(Z, gd, 1, 16, 64) == _stream(Z, gm, 1, 16, 64) == (0, want)
        assert _stream(Z, rd, 0, 128 << 10, 1 << 20) == _stream(Z, rm, 0, 128 << 10, 1 << 20) == (0, plains[0])
        # copied: entries 1..3 from the device reader into a heap writer are the archive the memory reader gives
        copies = []
        for r in (rm, rd):
            w = Writer()
            assert Z.lib.zpack_init_writer_heap(C.byref(w), 0) == 0
            assert Z.lib.zpack_write_header(C.byref(w)) == 0 and Z.lib.zpack_write_data_header(C.byref(w)) == 0
            assert Z.lib.zpack_write_files_from_archive(C.byref(w), C.byref(r), C.pointer(r.file_entries[1]), 3) == 0
            assert Z.lib.zpack_write_cdr(C.byref(w)) == 0 and Z.lib.zpack_write_eocdr(C.byref(w)) == 0
            copies.append(bytes(C.cast(w.buffer, C.POINTER(C.c_uint8 * w.file_size)).contents))
            Z.lib.zpack_close_writer(C.byref(w))
        assert copies[0] == copies[1]
        got = zpk.parse(copies[1])
        assert [(e["comp_size"], e["uncomp_size"], e["hash"], e["method"]) for e in got] == [(e["comp_size"], e["uncomp_size"], e["hash"], e["method"]) for e in pe[1:]]
        for e, src in zip(got, pe[1:]):
            assert copies[1][e["offset"]:e["offset"] + e["comp_size"]] == arc[src["offset"]:src["offset"] + src["comp_size"]]
    finally:
        for r in (gd, gm, rd, rm):
            Z.lib.zpack_close_reader(C.byref(r))


# ------------------------------------------------------------------------------------------------ 5. sub-batches

def test_sub_batches_by_the_chunk_option(torch, mixed):
    arc, order = mixed["arc"], mixed["order"]
    desc = _desc_of(arc)[order]
    desc["dst_capacity"] = mixed["caps"]
    t, at = _image(torch, arc, 1)
    image = t[1:1 + len(arc)]
    codec = zpack_amd.Codec(0)
    res0, outs0 = codec.decode_batch_dimage(image, desc)
    assert codec.dimage_stats()["sub_batches"] == 1 and (res0["status"] == 0).all()
    assert [o[:len(mixed["plains"][i])].tobytes() for o, i in zip(outs0, order)] == [mixed["plains"][i] for i in order]
    chunk = 1 << 20
    want, total, cnt = 0, 0, 0                                                         # the rule of include/zpack_codec.h, restated
    for d in desc:
        stored = int(d["method"]) == 0 and int(d["uncomp_size"]) < int(d["dst_capacity"])
        slot = ((int(d["uncomp_size"]) if stored else int(d["dst_capacity"])) + 255) & ~255
        if cnt and total + slot > chunk:
            want, total, cnt = want + 1, 0, 0
        total, cnt = total + slot, cnt + 1
    want += 1
    assert want > 1
    codec.set_option(zpack_amd.OPT_DIMAGE_CHUNK, chunk)
    res1, outs1 = codec.decode_batch_dimage(image, desc)
    s1 = codec.dimage_stats()
    offs, total = _layout(mixed["caps"], (1, 7, 15))
    buf = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda:0")
    res2 = codec.decode_batch_dimage(image, desc, [buf.data_ptr() + o for o in offs])
    s2 = codec.dimage_stats()
    print("sub-batches at 1 MiB: %d (restated: %d); %s, %s" % (s1["sub_batches"], want, s1, s2))
    assert s1["sub_batches"] == want and s2["sub_batches"] == want and s2["span_copy_launches"] == want and s1["span_copy_launches"] == 0
    assert res1.tobytes() == res0.tobytes() and res2.tobytes() == res0.tobytes()
    assert [o.tobytes() for o in outs1] == [o.tobytes() for o in outs0]
    got = _host_copy(torch, buf)
    want_buf = np.full(total, CANARY, dtype=np.uint8)
    for o, i in zip(offs, order):
        want_buf[o:o + len(mixed["plains"][i])] = np.frombuffer(mixed["plains"][i], dtype=np.uint8)
    assert np.array_equal(got, want_buf)
    codec.set_option(zpack_amd.OPT_DIMAGE_CHUNK, 0)                                    # 0 = the default again
    codec.decode_batch_dimage(image, desc[:5])
    assert codec.dimage_stats()["sub_batches"] == 1
    codec.close()


# ------------------------------------------------------------------------------------------------ 6. bad images

def _not_loaded(Z, r):
    """a batch read and a raw read on the reader (the raw read of an entry without bytes: no guard answers before the reader is asked)"""
    e, none = FileEntry(b"x", 10, 5, 5, 0, 0), FileEntry(b"y", 0, 0, 0, 0, 0)
    out = (C.c_uint8 * 16)()
    res = (C.c_int * 1)(-1)
    return (Z.lib.zpack_read_files(C.byref(r), (PFE * 1)(C.pointer(e)), 1, (C.c_void_p * 1)(C.addressof(out)), (C.c_size_t * 1)(16), res, None),
            Z.lib.zpack_read_raw_file(C.byref(r), C.pointer(none), C.addressof(out), 16))


def test_bad_images(Z, torch, golden_dir):
    arc = open(os.path.join(golden_dir, "ref_workdir", "archive_lz4.zpk"), "rb").read()
    t, at = _image(torch, arc)
    host = (C.c_uint8 * len(arc)).from_buffer_copy(arc)
    for image_at, size in ((C.addressof(host), len(arc)), (at, 1 << 40), (at + len(arc), 1 << 40)):
        r = Reader()
        assert Z.lib.zpack_amd_init_reader_device(C.byref(r), image_at, size) == STREAM_INVALID
        assert bytes(r) == bytes(C.sizeof(Reader))                                     # turned down before anything was copied or parsed
        assert _not_loaded(Z, r) == (NOT_LOADED,) * 2
    r = Reader()
    assert Z.lib.zpack_amd_init_reader_device(C.byref(r), None, len(arc)) == STREAM_INVALID                 # NULL with bytes
    assert bytes(r) == bytes(C.sizeof(Reader)) and _not_loaded(Z, r) == (NOT_LOADED,) * 2
    # ... and the device destinations of a batch read from a good image: NULL with bytes, a host address, a destination that leaves its
    # allocation are turned down before anything runs; no bytes pass wherever they point; the next good call on the same reader reads
    rd, keep = _open_dev(Z, torch, arc)
    ents = [rd.file_entries[i] for i in range(rd.file_count) if rd.file_entries[i].uncomp_size > 0][:4]
    n, k = len(ents), len(ents) - 1
    caps = [int(e.uncomp_size) for e in ents]
    offs, total = _layout(caps, (0,))
    dst = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda:0")
    small = torch.full((4096,), CANARY, dtype=torch.uint8, device="cuda:0")
    hostbuf = np.full(max(caps) + 64, CANARY, dtype=np.uint8)
    torch.cuda.synchronize()

    def read(at, cap):
        addr = [dst.data_ptr() + o for o in offs[:k]] + [at]
        res = (C.c_int * n)(*([-1] * n))
        rc = Z.lib.zpack_amd_read_files_device(C.byref(rd), (PFE * n)(*[C.pointer(e) for e in ents]), n, (C.c_void_p * n)(*addr),
                                               (C.c_size_t * n)(*(caps[:k] + [cap])), res, None)
        torch.cuda.synchronize()
        return rc, list(res)

    for at, cap in ((None, caps[k]), (hostbuf.ctypes.data, caps[k]), (small.data_ptr() + 100, 1 << 40)):
        assert read(at, cap) == (STREAM_INVALID, [-1] * n)
        assert bool((dst == CANARY).all()) and bool((small == CANARY).all()) and bool((hostbuf == CANARY).all())
    if torch.cuda.device_count() > 1:                                                  # memory of another device than the image's
        other = torch.full((caps[k] + 64,), CANARY, dtype=torch.uint8, device="cuda:1")
        torch.cuda.synchronize(1)
        assert read(other.data_ptr(), caps[k]) == (STREAM_INVALID, [-1] * n)
        assert bool((dst == CANARY).all()) and bool((other == CANARY).all())
    for at in (None, hostbuf.ctypes.data):
        rc, res = read(at, 0)
        assert rc == 0 and res[:k] == [0] * k and res[k] == 12                         # (max_size 0 < uncomp_size: BUFFER_TOO_SMALL, as on every path)
        assert bool((hostbuf == CANARY).all())
    assert read(dst.data_ptr() + offs[k], caps[k]) == (0, [0] * n)
    Z.lib.zpack_close_reader(C.byref(rd))
    cdr = int.from_bytes(arc[-8:], "little")
    cases = {"41 bytes": arc[:41],
             "header signature": b"\0" + arc[1:],
             "data signature": arc[:6] + b"Q" + arc[7:],
             "eocdr signature": arc[:-12] + b"\0" + arc[-11:],
             "cdr offset past the end": arc[:-8] + (len(arc) + 5).to_bytes(8, "little"),
             "cdr signature": arc[:cdr] + b"\0" + arc[cdr + 1:],
             "cdr block size": arc[:cdr + 12] + (1 << 30).to_bytes(8, "little") + arc[cdr + 20:],
             "cdr entry count": arc[:cdr + 4] + (3).to_bytes(8, "little") + arc[cdr + 12:]}
    codes = {}
    for what, bad in cases.items():
        keep = (C.c_uint8 * len(bad)).from_buffer_copy(bad)
        rm = Reader()
        want = Z.lib.zpack_init_reader_memory_shared(C.byref(rm), C.cast(keep, u8p), len(bad))
        Z.lib.zpack_close_reader(C.byref(rm))
        tb, bat = _image(torch, bad)
        rd = Reader()
        got = Z.lib.zpack_amd_init_reader_device(C.byref(rd), bat, len(bad))
        codes[what] = got
        assert got == want and got != 0, (what, got, want)
        assert _not_loaded(Z, rd) == (NOT_LOADED,) * 2, what
        Z.lib.zpack_close_reader(C.byref(rd))
    assert codes["41 bytes"] == FILE_TOO_SMALL and codes["header signature"] == 6 and codes["eocdr signature"] == 6
    print("codes:", codes)


# ------------------------------------------------------------------------------------------------ 8. read-ahead

def test_in_order_read_file_loop_keeps_its_read_ahead(Z, torch):
    specs = [((dg.LZ4, 0), (dg.ZSTD, 3), (dg.NONE, 0))[i % 3] + (_plain(i, 1500 + 37 * i),) for i in range(40)]
    arc = _build(specs)
    rm, keep = _open_mem(Z, arc)
    rd, image = _open_dev(Z, torch, arc, 7)
    try:
        got = {}
        for r in (rm, rd):
            outs = []
            for i in range(40):
                n = len(specs[i][2])
                out = np.full(n + GAP, CANARY, dtype=np.uint8)
                rc = Z.lib.zpack_read_file(C.byref(r), C.pointer(r.file_entries[i]), out.ctypes.data, n, None)
                outs.append((rc, int(r.last_return), out.tobytes()))
            got[id(r)] = outs
            stats = (C.c_uint64 * 6)()
            assert Z.lib.zpack_amd_read_ahead_stats(C.byref(r), None, stats) == 0
            assert stats[0] > 0 and stats[2] > 0, list(stats)                          # calls served from windows the context decoded
        assert got[id(rd)] == got[id(rm)]
        assert [o[2][:len(s[2])] for o, s in zip(got[id(rd)], specs)] == [s[2] for s in specs] and all(o[0] == 0 for o in got[id(rd)])
    finally:
        Z.lib.zpack_close_reader(C.byref(rd))
        Z.lib.zpack_close_reader(C.byref(rm))


# ------------------------------------------------------------------------------------------------ 9. lifetime and contexts

def test_close_leaves_the_image_and_the_struct_is_reusable(Z, torch, golden_dir):
    arc = open(os.path.join(golden_dir, "ref_workdir", "archive_zstd.zpk"), "rb").read()
    t, at = _image(torch, arc, 1)
    r = Reader()
    assert Z.lib.zpack_amd_init_reader_device(C.byref(r), at, len(arc)) == 0
    assert _read(Z, torch, r, [0, 1], [169, 349], "host")[0][:2] == (0, [0, 0])
    Z.lib.zpack_close_reader(C.byref(r))
    assert bytes(r) == bytes(C.sizeof(Reader)) and _not_loaded(Z, r) == (NOT_LOADED,) * 2
    assert t.cpu().numpy().tobytes() == b"\xEE" + arc + b"\xEE" * 3                     # not freed, not written
    keep = (C.c_uint8 * len(arc)).from_buffer_copy(arc)
    assert Z.lib.zpack_init_reader_memory_shared(C.byref(r), C.cast(keep, u8p), len(arc)) == 0      # the same struct, now a memory reader
    p, dev = C.c_void_p(1), C.c_int(0)
    assert Z.lib.zpack_amd_reader_device_image(C.byref(r), C.byref(p), C.byref(dev)) == 0 and (p.value, dev.value) == (None, -1)
    assert _read(Z, torch, r, [0, 1], [169, 349], "device")[0][:2] == (0, [0, 0])
    Z.lib.zpack_close_reader(C.byref(r))
    assert Z.lib.zpack_amd_init_reader_device(C.byref(r), at, len(arc)) == 0             # ... and a device reader again
    assert _read(Z, torch, r, [1], [349], "device")[0][:2] == (0, [0])
    Z.lib.zpack_close_reader(C.byref(r))


def test_explicit_contexts_and_two_threads_on_one_reader(Z, torch, mixed, mixed_ref):
    rd, image = _open_dev(Z, torch, mixed["arc"])
    ctxs = [Z.lib.zpack_create_dctx(METHOD_LZ4) for _ in range(2)]
    assert all(ctxs)
    try:
        order, caps = mixed["order"], mixed["caps"]
        half = len(order) // 2
        parts = [(order[:half], caps[:half]), (order[half:], caps[half:])]
        got = _read(Z, torch, rd, parts[0][0], parts[0][1], "device", (1, 7, 15), dctx=ctxs[0])      # an explicit dctx, on its own
        assert got[0][:2] == (0, [0] * half) and not rd.zstd_dctx                       # (the reader made no context of its own)
        out = [None, None]

        def work(k):
            torch.cuda.set_device(0)
            out[k] = [_read(Z, torch, rd, parts[k][0], parts[k][1], w, (1, 7, 15), dctx=ctxs[k]) for w in ("host", "device")]

        th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        for k in range(2):
            assert out[k] is not None
            for (rc, res, last), buf, offs in out[k]:
                assert (rc, res) == (0, [0] * len(parts[k][0]))
                want = np.full(len(buf), CANARY, dtype=np.uint8)
                for i, o in zip(parts[k][0], offs):
                    want[o:o + len(mixed["plains"][i])] = np.frombuffer(mixed["plains"][i], dtype=np.uint8)
                assert np.array_equal(buf, want)
    finally:
        Z.lib.zpack_close_reader(C.byref(rd))
        for c in ctxs:
            Z.lib.zpack_free_dctx(METHOD_LZ4, c)


# ------------------------------------------------------------------------------------------------ 10. the Python view

def test_device_io_reads_an_image_tensor(torch, mixed):
    from zpack_amd import device_io
    t, at = _image(torch, mixed["arc"], 0)
    image = t[:len(mixed["arc"])]
    out, status = device_io.read_files_device(image)
    assert status == [0] * len(mixed["plains"]) and len(out) == len(mixed["plains"])
    for got, want in zip(out, mixed["plains"]):
        assert got.is_cuda and got.dtype == torch.uint8 and got.device == image.device and got.cpu().numpy().tobytes() == want
    some, st = device_io.read_files_device(image, names=["e0017", "e0003"])
    assert st == [0, 0] and [x.cpu().numpy().tobytes() for x in some] == [mixed["plains"][17], mixed["plains"][3]]
    with pytest.raises(ValueError):
        device_io.read_files_device(image.to(torch.int8))
