"""GPU: delta entries through the library (include/zpack_amd.h: zpack_amd_write_files_device_delta, zpack_amd_read_files_device_delta), the
codec calls behind them and the torch view (zpack_amd/device_io.py), stored, LZ4 and Zstandard level 1, heap writer and device sink,
memory reader and device image.

The archive is that of tests/test_gpu_planes_io.py — twelve small bf16, fp32 and fp64 tensors, a uint8 entry with element size 1, an
empty entry, a 1 003-byte entry with element size 4 and a tail, one bf16 entry of 3 MiB that is written in pieces and read
block-parallel —, every entry with bytes against a base that differs from it in one byte of twenty.  The reference of every write is
zpack_amd_write_files_device_planes from device buffers that hold plain XOR base: the same image byte for byte.  The reference of every
read is the plain read of the same entries: its results, return value and last_return, and the bytes are the tensors — or what the buffer
held before, 0xA5 or, in place, the base."""
import ctypes as C
import json

import numpy as np
import pytest

import zpack_amd
from zpack_amd import device_io
from tests._libs import Reader, Writer, File, FileEntry, CompressOptions, u8p, oracle, have_ref, ref, METHOD_ZSTD, METHOD_LZ4
from tests.device_mem import torch, Z, _layout, CANARY, GAP            # noqa: F401  (torch, Z: fixtures)
from tests.test_gpu_planes_io import grouped, plain, _on_device, Opened, _want, _same, MIS, PFE      # noqa: F401  (plain: a fixture)

pytestmark = pytest.mark.gpu

OK, HASH_MISMATCH, STREAM_INVALID = 0, 15, 21
METHODS = [pytest.param((0, 0), id="stored"), pytest.param((METHOD_LZ4, 0), id="lz4"), pytest.param((METHOD_ZSTD, 1), id="zstd1")]


@pytest.fixture(scope="module")
def D(Z):
    """the library with the prototypes of the planes calls and the two new ones"""
    L = Z.lib
    R, W, vp, u64 = C.POINTER(Reader), C.POINTER(Writer), C.c_void_p, C.c_uint64
    L.zpack_amd_write_files_device_planes.argtypes = [W, C.POINTER(File), u64, C.POINTER(C.c_uint8)]
    L.zpack_amd_read_files_device_planes.argtypes = [R, C.POINTER(PFE), u64, vp, C.POINTER(C.c_size_t), C.POINTER(C.c_uint8), C.POINTER(C.c_int), vp]
    L.zpack_amd_write_files_device_delta.argtypes = [W, C.POINTER(File), u64, C.POINTER(C.c_uint8), C.POINTER(vp)]
    L.zpack_amd_read_files_device_delta.argtypes = [R, C.POINTER(PFE), u64, vp, C.POINTER(C.c_size_t), C.POINTER(C.c_uint8), C.POINTER(vp), C.POINTER(C.c_int), vp]
    L.zpack_amd_test_files.argtypes = [R, C.POINTER(PFE), u64, C.POINTER(C.c_int), vp]
    return Z


@pytest.fixture(scope="module")
def data(plain):
    """names, element sizes, the tensors' bytes and their bases: the tensor with one byte of twenty replaced, seeded; computed once"""
    rng = np.random.default_rng(29)
    bases = []
    for _, _, a in plain:
        b = a.copy()
        hit = rng.random(a.size) < 0.05
        b[hit] = rng.integers(0, 256, int(hit.sum()), dtype=np.uint8)
        bases.append(b)
    return dict(names=[p[0] for p in plain], elem=[p[1] for p in plain], arrays=[p[2] for p in plain], bases=bases)


def _write(D, torch, names, arrays, mc, elem, bases, sink, call="delta"):
    """header, data signature, the entries out of device memory, CDR, EOCDR -> (rc of the files call, the image's bytes, the entries'
    (offset, comp_size, uncomp_size, hash, method), write_offset before and behind the files call).  bases: arrays or None per entry (a
    number: that address as it is), or None for no base array at all.  Sources and bases are checked to be as they were."""
    L = D.lib
    n = len(names)
    buf, addr, before = _on_device(torch, arrays)
    c_bases = None
    if bases is not None:
        real = [b if isinstance(b, np.ndarray) else np.zeros(0, dtype=np.uint8) for b in bases]
        bbuf, baddr, bbefore = _on_device(torch, real, mis=(15, 0, 3, 1))
        c_bases = (C.c_void_p * n)(*[b if isinstance(b, int) else x for b, x in zip(bases, baddr)])
    opts = CompressOptions(*mc)
    arr = (File * n)()
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
        c_elem = None if elem is None else (C.c_uint8 * n)(*elem)
        if call == "delta":
            rc = L.zpack_amd_write_files_device_delta(C.byref(w), arr, n, c_elem, c_bases)
        else:
            assert bases is None
            rc = L.zpack_amd_write_files_device_planes(C.byref(w), arr, n, c_elem)
        at1 = int(w.write_offset)
        ents = [(int(e.offset), int(e.comp_size), int(e.uncomp_size), int(e.hash), int(e.comp_method)) for e in (w.file_entries[i] for i in range(w.file_count))]
        assert L.zpack_write_cdr(C.byref(w)) == 0 and L.zpack_write_eocdr(C.byref(w)) == 0
        torch.cuda.synchronize()
        image = C.string_at(w.buffer, w.file_size) if sink == "heap" else image_t[:int(w.file_size)].cpu().numpy().tobytes()
        assert np.array_equal(buf.cpu().numpy(), before)                                # sources and bases are read, never written
        assert bases is None or np.array_equal(bbuf.cpu().numpy(), bbefore)
        return rc, image, ents, (at0, at1)
    finally:
        L.zpack_close_writer(C.byref(w))


def _stored(arrays, elem, bases):
    return [grouped(a ^ b if isinstance(b, np.ndarray) else a, k) for a, k, b in zip(arrays, elem, bases)]


@pytest.fixture(scope="module", params=METHODS)
def made(request, D, torch, data):
    """one method: the image written by the delta call into a heap writer, its entries, and everything the tests share"""
    mc = request.param
    rc, image, ents, _ = _write(D, torch, data["names"], data["arrays"], mc, data["elem"], data["bases"], "heap")
    assert rc == OK and len(ents) == len(data["names"])
    return dict(data, mc=mc, stored=_stored(data["arrays"], data["elem"], data["bases"]), image=image, ents=ents)


def _read(D, torch, o, ents, caps, elem, bases, call="delta", inplace=False):
    """-> (rc, results, last_return), the whole destination buffer as it is afterwards, the destinations' offsets.  bases: arrays or None
    per entry (a number: that address as it is; a callable: of the destination's address), or None for no base array.  inplace: the
    destinations hold the bases' bytes and ARE the bases.  The bases elsewhere are checked to be as they were."""
    n = len(ents)
    offs, total = _layout(caps, MIS)
    h = np.full(total, CANARY, dtype=np.uint8)
    real = [b if isinstance(b, np.ndarray) else None for b in (bases or [None] * n)]
    if inplace:
        for x, b in zip(offs, real):
            if b is not None:
                h[x:x + b.size] = b
    buf = torch.from_numpy(h).to("cuda:0")
    torch.cuda.synchronize()
    dst = [buf.data_ptr() + x for x in offs]
    addr = (C.c_void_p * n)(*dst)
    c_bases = None
    if bases is not None:
        bbuf, baddr, bbefore = _on_device(torch, [b if b is not None else np.zeros(0, dtype=np.uint8) for b in real], mis=(1, 15, 0, 3))
        pick = []
        for b, x, d in zip(bases, baddr, dst):
            pick.append(b(d) if callable(b) else b if isinstance(b, int) else (d if inplace and b is not None else x))
        c_bases = (C.c_void_p * n)(*pick)
    ptrs = (PFE * n)(*[C.pointer(e) for e in ents])
    res = (C.c_int * n)(*([-1] * n))
    csz = (C.c_size_t * n)(*caps)
    c_elem = None if elem is None else (C.c_uint8 * n)(*elem)
    if call == "delta":
        rc = D.lib.zpack_amd_read_files_device_delta(C.byref(o.r), ptrs, n, addr, csz, c_elem, c_bases, res, None)
    elif call == "planes":
        rc = D.lib.zpack_amd_read_files_device_planes(C.byref(o.r), ptrs, n, addr, csz, c_elem, res, None)
    else:
        rc = D.lib.zpack_amd_read_files_device(C.byref(o.r), ptrs, n, addr, csz, res, None)
    torch.cuda.synchronize()
    assert bases is None or np.array_equal(bbuf.cpu().numpy(), bbefore)
    return (rc, list(res), int(o.r.last_return)), buf.cpu().numpy(), offs


# ------------------------------------------------------------------------------------------------ writes

def test_the_archive_is_the_planes_archive_of_buffers_that_hold_the_xor(D, torch, made):
    m = made
    rc, dimage, dents, _ = _write(D, torch, m["names"], m["arrays"], m["mc"], m["elem"], m["bases"], "device")
    assert rc == OK and dimage == m["image"] and dents == m["ents"]
    xored = [a ^ b for a, b in zip(m["arrays"], m["bases"])]
    for sink in ("heap", "device"):
        rc, pimage, pents, _ = _write(D, torch, m["names"], xored, m["mc"], m["elem"], None, sink, call="planes")
        assert rc == OK and pimage == m["image"] and pents == m["ents"], sink
    if m["mc"][0]:                                                                      # a twentieth of the bytes differ: the delta archive is the smaller one by far
        rc, full, _, _ = _write(D, torch, m["names"], m["arrays"], m["mc"], m["elem"], None, "heap", call="planes")
        assert rc == OK and len(m["image"]) * 2 < len(full)


def test_no_bases_is_the_planes_call_and_mixed_batches_base_some(D, torch, made):
    m = made
    names, arrays, elem = m["names"][:14], m["arrays"][:14], m["elem"][:14]
    rc, a, ea, _ = _write(D, torch, names, arrays, m["mc"], elem, None, "heap", call="planes")
    assert rc == OK
    for bases in (None, [None] * 14):                                                   # no base array; an array of no bases
        for sink in ("heap", "device"):
            assert _write(D, torch, names, arrays, m["mc"], elem, bases, sink)[:3] == (rc, a, ea), sink
    # every other entry with a base, the big one too; without element sizes: the bare XOR
    n = len(m["names"])
    some = [b if i % 2 == 0 or i == n - 1 else None for i, b in enumerate(m["bases"])]
    for elem in (m["elem"], None):
        mixed = [a ^ b if b is not None else a for a, b in zip(m["arrays"], some)]
        rc, want, went, _ = _write(D, torch, m["names"], mixed, m["mc"], elem, None, "heap", call="planes")
        for sink in ("heap", "device"):
            rc2, got, gent, _ = _write(D, torch, m["names"], m["arrays"], m["mc"], elem, some, sink)
            assert rc == OK and (rc2, got, gent) == (rc, want, went), sink
        for where in ("memory", "device"):
            o = Opened(D, torch, want, where)
            try:
                head, buf, offs = _read(D, torch, o, o.ents, [a.size for a in m["arrays"]], elem, some)
                assert head == (OK, [OK] * n, 0)
                _same(buf, _want(buf.size, offs, m["arrays"]), "mixed read")
            finally:
                o.close()


def test_the_oracle_and_the_reference_read_the_grouped_xor(made):
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


# ------------------------------------------------------------------------------------------------ reads

@pytest.mark.parametrize("where", ["memory", "device"])
def test_test_files_says_ok_and_the_delta_read_returns_the_tensors_in_place_too(D, torch, made, where):
    m = made
    o = Opened(D, torch, m["image"], where)
    try:
        n = len(o.ents)
        res = (C.c_int * n)(*([-1] * n))
        assert D.lib.zpack_amd_test_files(C.byref(o.r), (PFE * n)(*[C.pointer(e) for e in o.ents]), n, res, None) == OK and list(res) == [OK] * n
        caps = [a.size for a in m["arrays"]]
        head, buf, offs = _read(D, torch, o, o.ents, caps, m["elem"], m["bases"])
        assert head == (OK, [OK] * n, 0)
        _same(buf, _want(buf.size, offs, m["arrays"]), "delta read into fresh buffers")
        head, buf, offs = _read(D, torch, o, o.ents, caps, m["elem"], m["bases"], inplace=True)
        assert head == (OK, [OK] * n, 0)
        _same(buf, _want(buf.size, offs, m["arrays"]), "delta read in place")
        # without bases it is the planes call: the same results and the same bytes, which are the XOR
        headp, bufp, offs = _read(D, torch, o, o.ents, caps, m["elem"], None, call="planes")
        assert headp == head
        _same(bufp, _want(bufp.size, offs, [a ^ b for a, b in zip(m["arrays"], m["bases"])]), "planes read")
        for bases in (None, [None] * n):
            head1, buf1, _ = _read(D, torch, o, o.ents, caps, m["elem"], bases)
            assert head1 == head
            _same(buf1, bufp, "delta read without bases")
        # generous buffers, and a pick in another order: the bytes behind uncomp_size stay as they were
        pick = [n - 1, 3, 12, 0, 11, 13]
        ents = [o.ents[i] for i in pick]
        head2, buf2, offs2 = _read(D, torch, o, ents, [m["arrays"][i].size + 100 for i in pick], [m["elem"][i] for i in pick], [m["bases"][i] for i in pick])
        assert head2 == (OK, [OK] * len(pick), 0)
        _same(buf2, _want(buf2.size, offs2, [m["arrays"][i] for i in pick]), "a pick with room to spare")
    finally:
        o.close()


@pytest.mark.parametrize("where", ["memory", "device"])
def test_a_damaged_entry_has_the_plain_read_s_status_and_its_buffer_is_untouched(D, torch, made, where):
    m = made
    j = m["names"].index("fp32_4096")
    off, comp, unc, _, _ = m["ents"][j]
    cases = []
    if m["mc"][0]:
        broken = bytearray(m["image"]); broken[off] ^= 0xFF                            # the frame's first byte: no frame any more
        cases.append(("magic", bytes(broken), 0, True))
    broken = bytearray(m["image"]); broken[off + comp // 2] ^= 0xFF                    # somewhere inside: whatever the plain read says
    cases.append(("inside", bytes(broken), 0, False))
    cases.append(("comp_size", m["image"], 9, bool(m["mc"][0])))                       # the entry's last bytes are not its own (stored: whatever the plain read says)
    for what, image, cut, must_fail in cases:
        o = Opened(D, torch, image, where)
        try:
            mine = FileEntry.from_buffer_copy(o.ents[j])
            mine.comp_size -= cut
            ents = [o.ents[j - 1], mine, o.ents[j + 1]]
            idx = [j - 1, j, j + 1]
            caps = [m["arrays"][i].size for i in idx]
            elem = [m["elem"][i] for i in idx]
            bases = [m["bases"][i] for i in idx]
            headp, bufp, offs = _read(D, torch, o, ents, caps, None, None, call="plain")
            delivered = bufp[offs[1]:offs[1] + unc]
            for inplace in (False, True):
                head, buf, offs = _read(D, torch, o, ents, caps, elem, bases, inplace=inplace)
                assert head == headp, what                                              # results, return value, last_return: the plain read's
                assert head[1][0] == OK and head[1][2] == OK
                st = head[1][1]
                if must_fail:
                    assert st not in (OK, HASH_MISMATCH), (what, st)
                if st == OK or (st == HASH_MISMATCH and not bool((delivered[-8:] == CANARY).all())):
                    # (decoded to all of its bytes, right or wrong: the join of what the plain read delivers, XOR the base)
                    k, mm = elem[1], unc // elem[1]
                    middle = delivered.copy()
                    middle[:mm * k] = delivered[:mm * k].reshape(k, mm).T.reshape(-1)
                    middle ^= bases[1]
                else:
                    middle = bases[1] if inplace else None                              # untouched: its canaries, or still the previous checkpoint
                _same(buf, _want(buf.size, offs, [m["arrays"][j - 1], middle, m["arrays"][j + 1]]), (what, inplace))
        finally:
            o.close()


def test_a_bad_base_is_stream_invalid_and_nothing_moves(D, torch, made):
    m = made
    n = len(m["names"])
    big = n - 1                                                                         # 3 MiB: more than the allocator's block around a 4 KiB tensor holds
    small = torch.full((4096,), CANARY, dtype=torch.uint8, device="cuda:0")
    host = np.full(1 << 16, CANARY, dtype=np.uint8)
    torch.cuda.synchronize()
    for what, i, bad in (("host memory", 2, host.ctypes.data), ("too short", big, small.data_ptr())):
        bases = list(m["bases"]); bases[i] = bad
        for sink in ("heap", "device"):
            rc, image, ents, (at0, at1) = _write(D, torch, m["names"], m["arrays"], m["mc"], m["elem"], bases, sink)
            assert rc == STREAM_INVALID and at1 == at0 and ents == [], (what, sink)
    for where in ("memory", "device"):
        o = Opened(D, torch, m["image"], where)
        try:
            caps = [a.size for a in m["arrays"]]
            for what, i, bad in (("host memory", 2, host.ctypes.data), ("too short", big, small.data_ptr()),
                                 ("overlaps from behind", 10, lambda d: d + 2), ("overlaps from the front", 10, lambda d: d - 1),
                                 ("overlaps its last byte", big, lambda d: d + caps[big] - 1)):
                bases = list(m["bases"]); bases[i] = bad
                for inplace in (False, True):
                    head, buf, _ = _read(D, torch, o, o.ents, caps, m["elem"], bases, inplace=inplace)
                    assert head[0] == STREAM_INVALID and head[1] == [-1] * n, (what, where)
                    if not inplace:
                        assert bool((buf == CANARY).all()), (what, where)
        finally:
            o.close()
    assert bool((small == CANARY).all()) and bool((host == CANARY).all())


# ------------------------------------------------------------------------------------------------ what a base is worth

@pytest.mark.parametrize("mc", METHODS[1:])
def test_a_tensor_against_itself_compresses_to_nearly_nothing(D, torch, mc):
    """256 KiB of random bytes with the tensor as its own base: the stored bytes are all zero.  LZ4's format bound is 1/255, so a factor of
    20 is no measurement; without a base the same entry does not compress at all."""
    n = 256 << 10
    a = np.random.default_rng(255).integers(0, 256, n, dtype=np.uint8)
    for elem in ([2], None):
        rc, image, ents, _ = _write(D, torch, ["r"], [a], mc, elem, [a.copy()], "heap")
        assert rc == OK and ents[0][2] == n and ents[0][1] * 20 < n, (ents, elem)
        o = oracle()
        off, comp, unc, h, meth = ents[0]
        rc, out, got, hh = o.entry_decode(image, off, comp, unc, h, meth, unc)
        assert rc == OK and out[:unc] == bytes(n)
        rc, image, ents, _ = _write(D, torch, ["r"], [a], mc, elem, None, "heap")
        assert rc == OK and ents[0][1] >= n, (ents, elem)


# ------------------------------------------------------------------------------------------------ the torch view

@pytest.mark.parametrize("mc", METHODS[1:])
def test_device_io_round_trip_with_bases_in_place_and_the_manifest(torch, mc):
    g = torch.Generator().manual_seed(6)
    old = {
        "w.bf16": (torch.randn(300, 70, generator=g) * 0.02).to(torch.bfloat16).to("cuda:0"),
        "w.fp16": (torch.randn(4097, generator=g) * 0.02).to(torch.float16).to("cuda:0"),
        "w.fp32": (torch.randn(65537, generator=g) * 0.02).to("cuda:0"),
        "ids.int64": torch.arange(1000, dtype=torch.int64, device="cuda:0"),
        "mask.u8": (torch.arange(777, device="cuda:0") % 3).to(torch.uint8),
    }
    new = {k: t.clone() for k, t in old.items()}
    for k in ("w.bf16", "w.fp16", "w.fp32"):                                            # a step: one weight of sixteen moves a little
        flat = new[k].view(-1)
        flat[::16] = (flat[::16].float() * 1.01).to(flat.dtype)
    new["ids.int64"] += 1
    new["fresh.fp32"] = (torch.randn(129, generator=g) * 0.02).to("cuda:0")             # not in the previous checkpoint: no base
    base = {k: old[k] for k in ("w.bf16", "w.fp16", "w.fp32", "ids.int64")}
    raw = {k: t.contiguous().view(-1).view(torch.uint8).cpu().numpy().copy() for k, t in new.items()}
    old_raw = {k: t.contiguous().view(-1).view(torch.uint8).cpu().numpy().copy() for k, t in old.items()}
    image = device_io.write_archive_device(new, method=mc[0], level=mc[1], planes="dtype", base=base, base_id="step 7")
    assert device_io.write_files_device(None, new, method=mc[0], level=mc[1], planes="dtype", base=base, base_id="step 7") == image.cpu().numpy().tobytes()
    assert all(np.array_equal(t.contiguous().view(-1).view(torch.uint8).cpu().numpy(), old_raw[k]) for k, t in old.items())      # the bases are read only
    full = device_io.write_archive_device(new, method=mc[0], level=mc[1], planes="dtype")
    assert image.numel() < full.numel()
    # an ordinary archive to everyone else: both manifests are entries, the delta entries hold the grouped XOR
    outs, status = device_io.read_files_device(image)
    assert status == [OK] * (len(new) + 2) and device_io.test_files(image) == [OK] * (len(new) + 2)
    assert json.loads(outs[-1].cpu().numpy().tobytes().decode()) == {"entries": ["w.bf16", "w.fp16", "w.fp32", "ids.int64"], "base_id": "step 7"}
    assert np.array_equal(outs[0].cpu().numpy(), grouped(raw["w.bf16"] ^ old_raw["w.bf16"], 2))
    assert np.array_equal(outs[3].cpu().numpy(), raw["ids.int64"] ^ old_raw["ids.int64"])
    # through the manifests, into fresh tensors
    for archive in (image, image.cpu().numpy().tobytes()):
        outs, status = device_io.read_files_device(archive, planes="manifest", base=base, base_id="step 7")
        assert status == [OK] * len(new) and len(outs) == len(new)
        for (name, t), got in zip(new.items(), outs):
            assert np.array_equal(got.cpu().numpy(), raw[name]), name
    outs, status = device_io.read_files_device(image, names=["mask.u8", "w.fp32"], planes="manifest", base={"w.fp32": old["w.fp32"]})
    assert status == [OK, OK] and np.array_equal(outs[0].cpu().numpy(), raw["mask.u8"]) and np.array_equal(outs[1].cpu().numpy(), raw["w.fp32"])
    # a delta entry without its base is never handed out as if it were the tensor; another base than the recorded one is refused
    with pytest.raises(KeyError, match="w.fp16"):
        device_io.read_files_device(image, planes="manifest", base={k: v for k, v in base.items() if k != "w.fp16"})
    with pytest.raises(KeyError, match="w.bf16"):
        device_io.read_files_device(image, names=["w.bf16"], planes="manifest")
    outs, status = device_io.read_files_device(image, names=["mask.u8", "fresh.fp32"], planes="manifest")     # (no delta entry among them: no base needed)
    assert status == [OK, OK] and np.array_equal(outs[1].cpu().numpy(), raw["fresh.fp32"])
    with pytest.raises(ValueError, match="step 7"):
        device_io.read_files_device(image, planes="manifest", base=base, base_id="step 8")
    with pytest.raises(ValueError):
        device_io.write_archive_device(new, method=mc[0], level=mc[1], planes="dtype", base={"w.fp32": old["w.fp16"]})      # not the tensor's nbytes
    # in place: the previous checkpoint becomes the new one, and its tensors are what comes back
    outs, status = device_io.read_files_device(image, planes="manifest", base=base, base_id="step 7", inplace=True)
    assert status == [OK] * len(new)
    for (name, t), got in zip(new.items(), outs):
        if name in base:
            assert got is old[name] and torch.equal(old[name], t), name
        else:
            assert np.array_equal(got.cpu().numpy(), raw[name]), name


# ------------------------------------------------------------------------------------------------ the codec's counts

def test_delta_stats_count_rows_launches_and_staged_entries(D, torch, data):
    """the codec calls behind the library, LZ4: rows with a base are k_delta_copy's and counted by delta_stats, rows without one stay
    k_plane_copy's and planes_stats keeps its meaning; a large frame with a base and element size 1 is staged only because of its base"""
    mc = (METHOD_LZ4, 0)
    names, arrays, n = data["names"], data["arrays"], len(data["names"])
    big = n - 1
    elem = list(data["elem"]); elem[big] = 1                                            # the 3 MiB entry: the bare XOR
    some = [b if (i % 2 == 0 or i == big) and b.size else None for i, b in enumerate(data["bases"])]
    based = sum(1 for b in some if b is not None)
    unbased_grouped = sum(1 for a, k, b in zip(arrays, elem, some) if b is None and k > 1 and a.size)
    assert based == 9 and unbased_grouped == 6                                          # (even entries and the big one; the odd tensors)
    rc, image, ents, _ = _write(D, torch, names, arrays, mc, elem, some, "heap")
    assert rc == OK
    L = zpack_amd.lib()
    vp, u64 = C.c_void_p, C.c_uint64
    L.zpk_codec_encode_batch_dsink_delta.argtypes = [vp, vp, C.c_int, vp, u64, vp, u64, vp, C.POINTER(u64), C.POINTER(u64), vp, vp]
    L.zpk_codec_decode_batch_host_dptr_delta.argtypes = [vp, vp, u64, vp, u64, vp, vp, vp, vp]
    L.zpk_codec_decode_batch_dimage_delta.argtypes = [vp, vp, u64, vp, u64, vp, C.c_int, vp, vp, vp]
    codec = zpack_amd.Codec(0)
    try:
        buf, addr, _ = _on_device(torch, arrays)
        bbuf, baddr, _ = _on_device(torch, [b if b is not None else np.zeros(0, dtype=np.uint8) for b in some], mis=(3, 1, 15, 0))
        c_src = (vp * n)(*addr)
        c_base = (vp * n)(*baddr)
        c_elem = (C.c_uint8 * n)(*elem)
        # ---- writing into a sink ----
        desc = np.zeros(n, dtype=zpack_amd.ENCODE_DESC)
        desc["size"] = [a.size for a in arrays]
        desc["method"], desc["level"] = mc
        desc["dst_capacity"] = [codec.compress_bound(mc[0], a.size) for a in arrays]
        sink = torch.empty(int(desc["dst_capacity"].sum()) + 64, dtype=torch.uint8, device="cuda:0")
        res = np.zeros(n, dtype=zpack_amd.ENCODE_RESULT)
        placed, nbytes = u64(0), u64(0)
        torch.cuda.synchronize()
        assert L.zpk_codec_encode_batch_dsink_delta(codec.h, c_src, 1, desc.ctypes.data, n, sink.data_ptr(), sink.numel(), res.ctypes.data, C.byref(placed), C.byref(nbytes), c_elem, None) == 0
        assert codec.delta_stats() == dict(split=0, joined=0, launches=0, staged=0)     # no bases: what the planes call launches
        assert codec.planes_stats() == dict(split=sum(1 for a, k in zip(arrays, elem) if k > 1 and a.size), joined=0, launches=1, staged=0)
        assert L.zpk_codec_encode_batch_dsink_delta(codec.h, c_src, 1, desc.ctypes.data, n, sink.data_ptr(), sink.numel(), res.ctypes.data, C.byref(placed), C.byref(nbytes), c_elem, c_base) == 0
        assert placed.value == n and codec.delta_stats() == dict(split=based, joined=0, launches=1, staged=0)
        assert codec.planes_stats() == dict(split=unbased_grouped, joined=0, launches=1, staged=0)
        assert [int(h) for h in res["hash"]] == [e[3] for e in ents] and nbytes.value == sum(e[1] for e in ents)
        host = np.zeros(64, dtype=np.uint8)                                             # host sources take no base
        assert L.zpk_codec_encode_batch_dsink_delta(codec.h, (vp * 1)(host.ctypes.data), 0, desc[:1].ctypes.data, 1, sink.data_ptr(), sink.numel(), res.ctypes.data,
                                                    C.byref(placed), C.byref(nbytes), None, (vp * 1)(baddr[0])) == -2
        # ---- reading: the image in host memory, then in device memory ----
        dd = np.zeros(n, dtype=zpack_amd.DECODE_DESC)
        for i, (off, comp, unc, h, meth) in enumerate(ents):
            dd[i] = (off, comp, unc, h, 0, unc, meth, 0)
        offs, total = _layout([a.size for a in arrays], MIS)
        out = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda:0")
        c_dst = (vp * n)(*[out.data_ptr() + x for x in offs])
        want = _want(total, offs, arrays)
        arc = np.frombuffer(image, dtype=np.uint8)
        dres = np.zeros(n, dtype=zpack_amd.DECODE_RESULT)
        torch.cuda.synchronize()
        assert L.zpk_codec_decode_batch_host_dptr_delta(codec.h, arc.ctypes.data, arc.size, dd.ctypes.data, n, c_dst, dres.ctypes.data, c_elem, c_base) == 0
        torch.cuda.synchronize()
        ds, ps = codec.delta_stats(), codec.planes_stats()
        assert (dres["status"] == OK).all() and ds["split"] == 0 and ds["joined"] == based and ds["staged"] == 1 and ds["launches"] == 2      # the 3 MiB frame through the staging, one launch for the rest
        assert ps["split"] == 0 and ps["joined"] == unbased_grouped and ps["launches"] == ps["staged"] + 1      # (its own large frames through the staging, as before)
        _same(out.cpu().numpy(), want, "host image")
        image_t = torch.from_numpy(arc.copy()).to("cuda:0")
        out.fill_(CANARY)
        torch.cuda.synchronize()
        assert L.zpk_codec_decode_batch_dimage_delta(codec.h, image_t.data_ptr(), image_t.numel(), dd.ctypes.data, n, c_dst, 1, dres.ctypes.data, c_elem, c_base) == 0
        torch.cuda.synchronize()
        assert (dres["status"] == OK).all() and codec.delta_stats() == dict(split=0, joined=based, launches=1, staged=0)
        assert codec.planes_stats() == dict(split=0, joined=unbased_grouped, launches=1, staged=0)
        _same(out.cpu().numpy(), want, "device image")
        # host destinations take no base
        houts = [np.zeros(max(a.size, 1), dtype=np.uint8) for a in arrays]
        hp = (vp * n)(*[h.ctypes.data for h in houts])
        assert L.zpk_codec_decode_batch_dimage_delta(codec.h, image_t.data_ptr(), image_t.numel(), dd.ctypes.data, n, hp, 0, dres.ctypes.data, None, c_base) == -2
    finally:
        codec.close()
