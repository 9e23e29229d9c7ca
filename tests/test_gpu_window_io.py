"""GPU: window reads through the library (include/zpack_amd.h: zpack_amd_read_files_device_windows), the codec calls behind it and the
torch view (zpack_amd/device_io.py: read_files_device(..., window=)).

The archive is written with device_io from bf16, fp32 and uint8 tensors of 2-D and 3-D shapes, 64 KiB to 320 KiB each, LZ4; the 320 KiB
tensor is one frame and goes block-parallel on a reader in host memory.  It is written plain, with planes="dtype", and with bases, and
read on a memory reader, a file reader and a device image.  The reference of every window is the slice of the tensor that the whole
read delivers, made contiguous, byte for byte, between canaries.

A damaged entry: the statuses are zpack_amd_test_files'.  Its buffer is written when, and only when, the entry decoded to all of its
bytes (ZPACK_OK or ZPACK_ERROR_FILE_HASH_MISMATCH: the rule the delta and byte-plane reads have, include/zpack_amd.h), so an entry whose
hash FIELD alone is wrong delivers its window and one that does not decode leaves its buffer — in place, the base shard — as it was."""
import ctypes as C

import numpy as np
import pytest

import zpack_amd
from zpack_amd import device_io
from tests import zpk
from tests._libs import Reader, FileEntry, u8p, METHOD_LZ4
from tests.device_mem import torch, Z, _layout, CANARY, GAP            # noqa: F401  (torch, Z: fixtures)

pytestmark = pytest.mark.gpu

PFE = C.POINTER(FileEntry)
OK, BUFFER_TOO_SMALL, HASH_MISMATCH, STREAM_INVALID, BASE_MISMATCH = 0, 12, 15, 21, 64
MIS = (0, 1, 7, 15)
SHAPES = {"a.bf16": (128, 256), "b.fp32": (8, 33, 96), "c.u8": (5, 64, 1024), "d.bf16": (3, 40, 300)}
NAMES = list(SHAPES)
ELEM = {"a.bf16": 2, "b.fp32": 4, "c.u8": 1, "d.bf16": 2}
VARIANTS = ["plain", "planes", "delta"]
WHERE = ["memory", "file", "device"]


class Window(C.Structure):
    _fields_ = [("row_bytes", C.c_uint64), ("row0", C.c_uint64), ("rows", C.c_uint64), ("col0", C.c_uint64), ("cols", C.c_uint64)]


WHOLE = (0, 0, 0, 0, 0)


@pytest.fixture(scope="module")
def W(Z):
    L = Z.lib
    R, vp, u64 = C.POINTER(Reader), C.c_void_p, C.c_uint64
    L.zpack_amd_read_files_device_windows.argtypes = [R, C.POINTER(PFE), u64, vp, C.POINTER(C.c_size_t), C.POINTER(C.c_uint8), C.POINTER(vp), C.POINTER(u64),
                                                      C.POINTER(Window), C.POINTER(C.c_int), vp]
    L.zpack_amd_read_files_device_delta_checked.argtypes = [R, C.POINTER(PFE), u64, vp, C.POINTER(C.c_size_t), C.POINTER(C.c_uint8), C.POINTER(vp), C.POINTER(u64),
                                                            C.POINTER(C.c_int), vp]
    L.zpack_amd_test_files.argtypes = [R, C.POINTER(PFE), u64, C.POINTER(C.c_int), vp]
    L.zpack_init_reader.argtypes = [R, C.c_char_p]
    return Z


def _bytes(t):
    return t.contiguous().view(-1).view(dtype=device_io._u8()).cpu().numpy().copy()


@pytest.fixture(scope="module")
def ckpt(torch):
    """the tensors (`new`), the previous checkpoint (`old`: one weight of sixteen a little off), their bytes, and the three archives"""
    g = torch.Generator().manual_seed(34)
    new = {
        "a.bf16": (torch.randn(SHAPES["a.bf16"], generator=g) * 0.02).to(torch.bfloat16).to("cuda:0"),                                # 64 KiB
        "b.fp32": (torch.randn(SHAPES["b.fp32"], generator=g) * 0.02).to("cuda:0"),                                                   # 99 KiB
        "c.u8": ((torch.arange(5 * 64 * 1024, dtype=torch.int64) * 7 // 13) % 251).to(torch.uint8).reshape(SHAPES["c.u8"]).to("cuda:0"),   # 320 KiB: one frame, block-parallel
        "d.bf16": (torch.randn(SHAPES["d.bf16"], generator=g) * 0.02).to(torch.bfloat16).to("cuda:0"),                                # 70 KiB, rows of 600 bytes
    }
    old = {k: t.clone() for k, t in new.items()}
    for k in ("a.bf16", "b.fp32", "d.bf16"):
        flat = old[k].view(-1)
        flat[::16] = (flat[::16].float() * 1.01).to(flat.dtype)
    old["c.u8"] = old["c.u8"] ^ 3
    torch.cuda.synchronize()
    images = {
        "plain": device_io.write_files_device(None, new, method=METHOD_LZ4, level=0),
        "planes": device_io.write_files_device(None, new, method=METHOD_LZ4, level=0, planes="dtype"),
        "delta": device_io.write_files_device(None, new, method=METHOD_LZ4, level=0, planes="dtype", base=old),
    }
    for v, image in images.items():
        ents = zpk.parse(image)
        assert [e["filename"] for e in ents[:4]] == NAMES and all(e["method"] == METHOD_LZ4 for e in ents[:4]), v
        assert [e["uncomp_size"] for e in ents[:4]] == [65536, 101376, 327680, 72000]
    return dict(new=new, old=old, raw={k: _bytes(t) for k, t in new.items()}, old_raw={k: _bytes(t) for k, t in old.items()}, images=images)


class Opened:
    """a reader over the image: in host memory, a file, or in device memory; ents: the four tensors' entries"""
    def __init__(self, W, torch, image, where, tmp_path=None):
        self.L, self.r = W.lib, Reader()
        if where == "memory":
            self.keep = (C.c_uint8 * len(image)).from_buffer_copy(image)
            assert self.L.zpack_init_reader_memory_shared(C.byref(self.r), C.cast(self.keep, u8p), len(image)) == 0
        elif where == "file":
            path = tmp_path / "w.zpk"
            path.write_bytes(image)
            assert self.L.zpack_init_reader(C.byref(self.r), str(path).encode()) == 0
        else:
            self.keep = torch.from_numpy(np.frombuffer(image, dtype=np.uint8).copy()).to("cuda:0")
            torch.cuda.synchronize()
            assert self.L.zpack_amd_init_reader_device(C.byref(self.r), self.keep.data_ptr(), len(image)) == 0
        self.ents = [self.r.file_entries[i] for i in range(4)]

    def close(self):
        self.L.zpack_close_reader(C.byref(self.r))


def _window(name, dim, start, stop):
    return zpack_amd.slice_window(SHAPES[name], dim, start, stop, ELEM[name])


def _slice(raw, name, dim, start, stop):
    """bytes of the tensor -> bytes of its slice along dim, made contiguous"""
    a = raw.reshape(SHAPES[name] + (ELEM[name],))
    return np.ascontiguousarray(a[(slice(None),) * dim + (slice(start, stop),)]).reshape(-1)


def _call(W, torch, o, ents, caps, elem, wins, prefill=None, bases=None, hashes=None, inplace=False, call="windows", room=None):
    """one call into destinations between canaries.  prefill: what destination i holds beforehand (None: canaries); bases: np arrays (or
    None per entry), placed in a buffer of their own — inplace: the destination, which then holds them, IS the base; a number: that
    address; a callable: of the destination's address.  room: max_sizes, when they are not the buffers' sizes.
    -> (rc, results, last_return), the destination buffer afterwards, the offsets"""
    n = len(ents)
    offs, total = _layout(caps, MIS)
    h = np.full(total, CANARY, dtype=np.uint8)
    real = [b if isinstance(b, np.ndarray) else None for b in (bases or [None] * n)]
    for i, x in enumerate(offs):
        if inplace and real[i] is not None:
            h[x:x + real[i].size] = real[i]
        elif prefill is not None and prefill[i] is not None:
            h[x:x + prefill[i].size] = prefill[i]
    buf = torch.from_numpy(h).to("cuda:0")
    dst = [buf.data_ptr() + x for x in offs]
    c_bases = None
    if bases is not None:
        boffs, btotal = _layout([b.size if b is not None else 0 for b in real], (15, 7, 0, 1))
        bh = np.full(btotal, CANARY, dtype=np.uint8)
        for b, x in zip(real, boffs):
            if b is not None:
                bh[x:x + b.size] = b
        bbuf = torch.from_numpy(bh).to("cuda:0")
        pick = []
        for b, r_, x, d in zip(bases, real, boffs, dst):
            pick.append(b(d) if callable(b) else b if isinstance(b, int) else None if r_ is None else d if inplace else bbuf.data_ptr() + x)
        c_bases = (C.c_void_p * n)(*pick)
    torch.cuda.synchronize()
    ptrs = (PFE * n)(*[C.pointer(e) for e in ents])
    res = (C.c_int * n)(*([-1] * n))
    csz = (C.c_size_t * n)(*(room if room is not None else caps))
    c_elem = None if elem is None else (C.c_uint8 * n)(*elem)
    c_hash = None if hashes is None else (C.c_uint64 * n)(*hashes)
    addr = (C.c_void_p * n)(*dst)
    if call == "windows":
        c_win = None if wins is None else (Window * n)(*[Window(*w) for w in wins])
        rc = W.lib.zpack_amd_read_files_device_windows(C.byref(o.r), ptrs, n, addr, csz, c_elem, c_bases, c_hash, c_win, res, None)
    else:
        assert wins is None
        rc = W.lib.zpack_amd_read_files_device_delta_checked(C.byref(o.r), ptrs, n, addr, csz, c_elem, c_bases, c_hash, res, None)
    torch.cuda.synchronize()
    if bases is not None:
        assert np.array_equal(bbuf.cpu().numpy(), bh)                                  # bases elsewhere are only read
    return (rc, list(res), int(o.r.last_return)), buf.cpu().numpy(), offs


def _want(total, offs, parts):
    w = np.full(total, CANARY, dtype=np.uint8)
    for x, p in zip(offs, parts):
        if p is not None:
            w[x:x + p.size] = p
    return w


def _same(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, int(bad[0]), bad.size)


def _variant(ckpt, variant):
    """element sizes and the whole bases (bytes) of a variant"""
    elem = None if variant == "plain" else [ELEM[k] for k in NAMES]
    bases = [ckpt["old_raw"][k] for k in NAMES] if variant == "delta" else None
    return elem, bases


def _rounds():
    """per round: for each entry (dim, start, stop) or None = read whole.  Round r windows dimension r of every tensor that has one — the
    2-D tensors are read whole beside the windowed 3-D ones in round 2 —, at another place each round; a last round takes the first
    eighth along dimension 0 and the last eighth along the last dimension"""
    out = []
    for r in range(3):
        row = []
        for name in NAMES:
            shape = SHAPES[name]
            if r >= len(shape):
                row.append(None)
                continue
            size = shape[r]
            row.append((r, size // 3, size - size // 4) if r != 1 else (r, 1, size - 1))
        out.append(row)
    out.append([(0, 0, SHAPES[NAMES[0]][0] // 8), (2, 96 - 12, 96), (0, 4, 5), (2, 0, 300 // 8)])
    return out


# ------------------------------------------------------------------------------------------------ the windows

@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("variant", VARIANTS)
def test_every_window_along_every_dim_is_the_slice_of_the_whole_read(W, torch, ckpt, tmp_path, variant, where):
    elem, bases = _variant(ckpt, variant)
    o = Opened(W, torch, ckpt["images"][variant], where, tmp_path)
    try:
        sizes = [ckpt["raw"][k].size for k in NAMES]
        # windows == NULL is the _delta_checked call: results, last_return and bytes
        head0, buf0, offs0 = _call(W, torch, o, o.ents, sizes, elem, None, bases=bases, call="delta_checked")
        head1, buf1, _ = _call(W, torch, o, o.ents, sizes, elem, None, bases=bases)
        assert head0 == (OK, [OK] * 4, 0) and head1 == head0
        _same(buf1, buf0, "windows == NULL")
        _same(buf0, _want(buf0.size, offs0, [ckpt["raw"][k] for k in NAMES]), "the whole read")
        whole = [buf0[x:x + s] for x, s in zip(offs0, sizes)]                           # the reference: what the whole read delivered
        for ri, row in enumerate(_rounds()):
            wins, want, caps, wbases = [], [], [], []
            for name, cut, full, b in zip(NAMES, row, whole, bases or [None] * 4):
                wins.append(WHOLE if cut is None else _window(name, *cut))
                want.append(full if cut is None else _slice(full, name, *cut))
                wbases.append(None if b is None else b if cut is None else _slice(b, name, *cut))
                caps.append(want[-1].size)
            assert any(c is None for c in row) == (ri == 2)                             # one call mixes windowed and whole entries
            head, buf, offs = _call(W, torch, o, o.ents, caps, elem, wins, bases=wbases if bases else None)
            assert head == (OK, [OK] * 4, 0), (ri, head)
            _same(buf, _want(buf.size, offs, want), ("round", ri))
            if bases:                                                                   # in place: the shards of the previous checkpoint become the slices of the new one
                head, buf, offs = _call(W, torch, o, o.ents, caps, elem, wins, bases=wbases, inplace=True)
                assert head == (OK, [OK] * 4, 0), (ri, head)
                _same(buf, _want(buf.size, offs, want), ("round in place", ri))
        # a pick in another order, generous buffers: the bytes behind window_bytes stay as they were
        pick = [2, 0, 3]
        cuts = [(1, 3, 64), (1, 255, 256), (2, 1, 2)]
        wins = [_window(NAMES[i], *c) for i, c in zip(pick, cuts)]
        want = [_slice(whole[i], NAMES[i], *c) for i, c in zip(pick, cuts)]
        wb = [_slice(bases[i], NAMES[i], *c) for i, c in zip(pick, cuts)] if bases else None
        head, buf, offs = _call(W, torch, o, [o.ents[i] for i in pick], [w.size + 100 for w in want], None if elem is None else [elem[i] for i in pick], wins,
                                bases=wb)
        assert head == (OK, [OK] * 3, 0)
        _same(buf, _want(buf.size, offs, want), "a pick with room to spare")
    finally:
        o.close()


# ------------------------------------------------------------------------------------------------ verdicts

@pytest.mark.parametrize("where", WHERE)
def test_a_damaged_entry_has_the_status_of_test_files_and_is_delivered_whole_or_not_at_all(W, torch, ckpt, tmp_path, where):
    image = ckpt["images"]["delta"]
    ents = zpk.parse(image)
    elem, bases = _variant(ckpt, "delta")
    cut = {"a.bf16": (1, 64, 96), "b.fp32": (0, 2, 5), "c.u8": (2, 100, 228), "d.bf16": (1, 7, 9)}
    wins = [_window(k, *cut[k]) for k in NAMES]
    want = [_slice(ckpt["raw"][k], k, *cut[k]) for k in NAMES]
    shards = [_slice(b, k, *cut[k]) for k, b in zip(NAMES, bases)]
    caps = [w.size for w in want]
    for j in (1, 2):                                                                    # a one-wave entry and the block-parallel one
        e = ents[j]
        magic = bytearray(image); magic[e["offset"]] ^= 0xFF                            # the frame's first byte: no frame any more
        inside = bytearray(image); inside[e["offset"] + e["comp_size"] // 2] ^= 0xFF    # somewhere inside: whatever test_files says
        for what, img, wrong_hash, must_fail in (("magic", bytes(magic), False, True), ("inside", bytes(inside), False, False), ("hash field", image, True, False)):
            o = Opened(W, torch, img, where, tmp_path)
            try:
                mine = list(o.ents)
                if wrong_hash:
                    mine[j] = FileEntry.from_buffer_copy(o.ents[j])
                    mine[j].hash ^= 1
                res = (C.c_int * 4)(*([-1] * 4))
                assert W.lib.zpack_amd_test_files(C.byref(o.r), (PFE * 4)(*[C.pointer(x) for x in mine]), 4, res, None) == OK
                verdicts = list(res)
                assert verdicts[j] != OK and all(v == OK for i, v in enumerate(verdicts) if i != j), (what, verdicts)
                if must_fail:
                    assert verdicts[j] != HASH_MISMATCH, (what, verdicts)
                if wrong_hash:
                    assert verdicts[j] == HASH_MISMATCH
                # what decoded, when all of it did: the whole read of the same entries delivers it (and leaves canaries where it did not)
                sizes = [ckpt["raw"][k].size for k in NAMES]
                headw, bufw, offsw = _call(W, torch, o, mine, sizes, elem, None, bases=bases)
                assert headw[1] == verdicts
                full = bufw[offsw[j]:offsw[j] + sizes[j]]
                decoded_all = verdicts[j] == HASH_MISMATCH and not bool((full == CANARY).all())
                assert decoded_all or not wrong_hash
                for inplace in (False, True):
                    head, buf, offs = _call(W, torch, o, mine, caps, elem, wins, bases=shards, inplace=inplace)
                    assert head[0] == OK and head[1] == verdicts, (what, head, verdicts)
                    parts = list(want)
                    parts[j] = _slice(full, NAMES[j], *cut[NAMES[j]]) if decoded_all else shards[j] if inplace else None
                    _same(buf, _want(buf.size, offs, parts), (what, j, inplace))
            finally:
                o.close()


@pytest.mark.parametrize("where", WHERE)
def test_base_hashes_too_small_buffers_and_refusals(W, torch, ckpt, tmp_path, where):
    elem, bases = _variant(ckpt, "delta")
    cut = {"a.bf16": (0, 16, 32), "b.fp32": (2, 8, 24), "c.u8": (1, 60, 64), "d.bf16": (2, 150, 300)}
    wins = [_window(k, *cut[k]) for k in NAMES]
    want = [_slice(ckpt["raw"][k], k, *cut[k]) for k in NAMES]
    shards = [_slice(b, k, *cut[k]) for k, b in zip(NAMES, bases)]
    caps = [w.size for w in want]
    # the shards' hashes, on the device, as a reader would compute them
    good = device_io.hash_tensors([torch.from_numpy(s).to("cuda:0") for s in shards])
    o = Opened(W, torch, ckpt["images"]["delta"], where, tmp_path)
    try:
        head, buf, offs = _call(W, torch, o, o.ents, caps, elem, wins, bases=shards, hashes=good)
        assert head == (OK, [OK] * 4, 0)
        _same(buf, _want(buf.size, offs, want), "checked bases")
        # a wrong base_hashes[i]: BASE_MISMATCH, the destination untouched — in place it is the base shard
        wrong = list(good); wrong[1] ^= 1; wrong[2] ^= 1 << 40
        for inplace in (False, True):
            head, buf, offs = _call(W, torch, o, o.ents, caps, elem, wins, bases=shards, hashes=wrong, inplace=inplace)
            assert head[0] == OK and head[1] == [OK, BASE_MISMATCH, BASE_MISMATCH, OK]
            parts = [want[0], shards[1] if inplace else None, shards[2] if inplace else None, want[3]]
            _same(buf, _want(buf.size, offs, parts), ("wrong hash", inplace))
        # max_sizes[i] = window_bytes - 1: BUFFER_TOO_SMALL for that entry alone, nothing of it written
        for j in (0, 2):
            room = list(caps); room[j] -= 1
            head, buf, offs = _call(W, torch, o, o.ents, caps, elem, wins, bases=shards, hashes=good, room=room)
            assert head[0] == OK and head[1] == [BUFFER_TOO_SMALL if i == j else OK for i in range(4)], head
            _same(buf, _want(buf.size, offs, [None if i == j else w for i, w in enumerate(want)]), ("too small", j))
        # an invalid window, or a base that overlaps its buffer in part: STREAM_INVALID, nothing moved, no result set
        n2 = ckpt["raw"]["c.u8"].size
        for what, j, bad in (("a row too many", 2, (64 * 1024, 0, 6, 0, 64)), ("past the row's end", 2, (64 * 1024, 0, 5, 64 * 1024 - 32, 64)),
                             ("not whole elements", 1, (96 * 4, 0, 8 * 33, 2, 8)), ("no rows of the entry", 0, (500, 0, 1, 0, 2)),
                             ("wraps", 3, (600, 2 ** 64 - 1, 2, 0, 2))):
            w2 = list(wins); w2[j] = bad
            head, buf, _ = _call(W, torch, o, o.ents, caps, elem, w2, bases=shards, hashes=good)
            assert head[0] == STREAM_INVALID and head[1] == [-1] * 4, what
            assert bool((buf == CANARY).all()), what
        assert n2 % (64 * 1024) == 0
        for what, j, at in (("from behind", 1, lambda d: d + 4), ("from the front", 1, lambda d: d - 1), ("its last byte", 2, lambda d: d + caps[2] - 1)):
            b2 = list(shards); b2[j] = at
            head, buf, _ = _call(W, torch, o, o.ents, caps, elem, wins, bases=b2, hashes=None)
            assert head[0] == STREAM_INVALID and head[1] == [-1] * 4, what
            assert bool((buf == CANARY).all()), what
    finally:
        o.close()


# ------------------------------------------------------------------------------------------------ the codec: sub-batches and counts

def _codec_protos():
    L = zpack_amd.lib()
    vp, u64 = C.c_void_p, C.c_uint64
    L.zpk_codec_decode_batch_host_dptr_windows.argtypes = [vp, vp, u64, vp, u64, vp, vp, vp, vp, vp, vp]
    L.zpk_codec_decode_batch_dimage_windows.argtypes = [vp, vp, u64, vp, u64, vp, C.c_int, vp, vp, vp, vp, vp]
    L.zpk_codec_decode_batch_host_dptr_delta_checked.argtypes = [vp, vp, u64, vp, u64, vp, vp, vp, vp, vp]
    L.zpk_codec_decode_batch_dimage_delta_checked.argtypes = [vp, vp, u64, vp, u64, vp, C.c_int, vp, vp, vp, vp]
    return L


def _descs(image):
    ents = zpk.parse(image)[:4]
    dd = np.zeros(4, dtype=zpack_amd.DECODE_DESC)
    for i, e in enumerate(ents):
        dd[i] = (e["offset"], e["comp_size"], e["uncomp_size"], e["hash"], 0, e["uncomp_size"], e["method"], 0)
    return dd


def test_a_small_dimage_chunk_cuts_the_windows_with_their_sub_batches(torch, ckpt):
    L = _codec_protos()
    image = ckpt["images"]["delta"]
    elem, bases = _variant(ckpt, "delta")
    cut = {"a.bf16": (1, 5, 200), "b.fp32": (1, 3, 30), "c.u8": (0, 1, 4), "d.bf16": (2, 17, 290)}
    wins = np.array([_window(k, *cut[k]) for k in NAMES], dtype=zpack_amd.WINDOW)
    want = [_slice(ckpt["raw"][k], k, *cut[k]) for k in NAMES]
    shards = [_slice(b, k, *cut[k]) for k, b in zip(NAMES, bases)]
    caps = [w.size for w in want]
    dd = _descs(image)
    dd["dst_capacity"] = caps                                                           # the room at the destinations
    offs, total = _layout(caps, MIS)
    out = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda:0")
    boffs, btotal = _layout(caps, (7, 0, 15, 1))
    bh = np.zeros(btotal, dtype=np.uint8)
    for s, x in zip(shards, boffs):
        bh[x:x + s.size] = s
    bbuf = torch.from_numpy(bh).to("cuda:0")
    image_t = torch.from_numpy(np.frombuffer(image, dtype=np.uint8).copy()).to("cuda:0")
    c_dst = (C.c_void_p * 4)(*[out.data_ptr() + x for x in offs])
    c_base = (C.c_void_p * 4)(*[bbuf.data_ptr() + x for x in boffs])
    c_elem = (C.c_uint8 * 4)(*elem)
    res = np.zeros(4, dtype=zpack_amd.DECODE_RESULT)
    codec = zpack_amd.Codec(0)
    try:
        torch.cuda.synchronize()
        for chunk, subs in ((0, 1), (128 << 10, 4), (200 << 10, 3)):                    # slots of 64, 99, 320 and 70.5 KiB
            codec.set_option(zpack_amd.OPT_DIMAGE_CHUNK, chunk)
            out.fill_(CANARY)
            torch.cuda.synchronize()
            assert L.zpk_codec_decode_batch_dimage_windows(codec.h, image_t.data_ptr(), image_t.numel(), dd.ctypes.data, 4, c_dst, 1, res.ctypes.data, c_elem, c_base,
                                                           None, wins.ctypes.data) == 0
            torch.cuda.synchronize()
            assert (res["status"] == OK).all() and codec.dimage_stats()["sub_batches"] == subs, (chunk, codec.dimage_stats())
            assert codec.window_stats() == dict(rows=4, launches=subs, staged=0)
            _same(out.cpu().numpy(), _want(total, offs, want), chunk)
        # host destinations take no window
        houts = [np.zeros(c, dtype=np.uint8) for c in caps]
        hp = (C.c_void_p * 4)(*[h.ctypes.data for h in houts])
        assert L.zpk_codec_decode_batch_dimage_windows(codec.h, image_t.data_ptr(), image_t.numel(), dd.ctypes.data, 4, hp, 0, res.ctypes.data, None, None, None, wins.ctypes.data) == -2
    finally:
        codec.close()


def test_window_stats_count_rows_launches_and_the_staged_frame_and_leave_the_other_counts_alone(torch, ckpt):
    """the codec calls behind the library: rows with a window are k_window_copy's, whatever their element size or base; the 320 KiB frame,
    read block-parallel from an image in host memory, is staged only because of its window; a batch without windows launches and counts
    exactly what the _delta_checked call does"""
    L = _codec_protos()
    codec = zpack_amd.Codec(0)
    try:
        for variant in VARIANTS:
            image = ckpt["images"][variant]
            elem, bases = _variant(ckpt, variant)
            sizes = [ckpt["raw"][k].size for k in NAMES]
            dd = _descs(image)
            arc = np.frombuffer(image, dtype=np.uint8)
            image_t = torch.from_numpy(arc.copy()).to("cuda:0")
            offs, total = _layout(sizes, MIS)
            out = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda:0")
            c_dst = (C.c_void_p * 4)(*[out.data_ptr() + x for x in offs])
            c_elem = None if elem is None else (C.c_uint8 * 4)(*elem)
            c_base = bbuf = None
            if bases:
                bbuf = torch.from_numpy(np.concatenate([np.concatenate([b, np.zeros(-b.size % 256, dtype=np.uint8)]) for b in bases])).to("cuda:0")
                starts = np.cumsum([0] + [b.size + (-b.size % 256) for b in bases[:-1]])
                c_base = (C.c_void_p * 4)(*[bbuf.data_ptr() + int(s) for s in starts])
            res = np.zeros(4, dtype=zpack_amd.DECODE_RESULT)
            whole_rows = np.array([WHOLE] * 4, dtype=zpack_amd.WINDOW)
            torch.cuda.synchronize()

            def counts():
                return codec.planes_stats(), codec.delta_stats(), codec.window_stats(), codec.decode_stats()["span_copy_launches"]

            # ---- no windows: NULL, and an array of no windows, against the _delta_checked call ----
            assert L.zpk_codec_decode_batch_host_dptr_delta_checked(codec.h, arc.ctypes.data, arc.size, dd.ctypes.data, 4, c_dst, res.ctypes.data, c_elem, c_base, None) == 0
            torch.cuda.synchronize()
            ref_counts, ref_res, ref_out = counts(), res.copy(), out.cpu().numpy()
            assert (ref_res["status"] == OK).all() and ref_counts[2] == dict(rows=0, launches=0, staged=0)
            # (what that call has always left: the 320 KiB frame goes block-parallel — straight into its destination, through the staging
            # when it has a base —, the three others are one launch of the kernel their kind takes)
            zero = dict(split=0, joined=0, launches=0, staged=0)
            assert ref_counts[:2] + ref_counts[3:] == {"plain": (zero, zero, 1), "planes": (dict(zero, joined=3, launches=1), zero, 0),
                                                       "delta": (zero, dict(zero, joined=4, launches=2, staged=1), 0)}[variant], (variant, ref_counts)
            for win in (None, whole_rows.ctypes.data):
                out.fill_(CANARY)
                torch.cuda.synchronize()
                assert L.zpk_codec_decode_batch_host_dptr_windows(codec.h, arc.ctypes.data, arc.size, dd.ctypes.data, 4, c_dst, res.ctypes.data, c_elem, c_base, None, win) == 0
                torch.cuda.synchronize()
                assert counts() == ref_counts and res.tobytes() == ref_res.tobytes(), variant
                _same(out.cpu().numpy(), ref_out, (variant, "no windows"))
            assert L.zpk_codec_decode_batch_dimage_delta_checked(codec.h, image_t.data_ptr(), image_t.numel(), dd.ctypes.data, 4, c_dst, 1, res.ctypes.data, c_elem, c_base, None) == 0
            torch.cuda.synchronize()
            ref_counts = counts()
            assert L.zpk_codec_decode_batch_dimage_windows(codec.h, image_t.data_ptr(), image_t.numel(), dd.ctypes.data, 4, c_dst, 1, res.ctypes.data, c_elem, c_base, None, whole_rows.ctypes.data) == 0
            torch.cuda.synchronize()
            assert counts() == ref_counts and res.tobytes() == ref_res.tobytes(), variant
            # ---- windows on three of the four, the block-parallel frame among them; the base of a window is its shard ----
            cut = {"a.bf16": None, "b.fp32": (2, 0, 12), "c.u8": (0, 2, 3), "d.bf16": (1, 0, 40)}
            wins = np.array([WHOLE if cut[k] is None else _window(k, *cut[k]) for k in NAMES], dtype=zpack_amd.WINDOW)
            want = [ckpt["raw"][k] if cut[k] is None else _slice(ckpt["raw"][k], k, *cut[k]) for k in NAMES]
            if bases:
                shards = [b if cut[k] is None else _slice(b, k, *cut[k]) for k, b in zip(NAMES, bases)]
                sbuf = torch.from_numpy(np.concatenate([np.concatenate([b, np.zeros(-b.size % 256, dtype=np.uint8)]) for b in shards])).to("cuda:0")
                starts = np.cumsum([0] + [b.size + (-b.size % 256) for b in shards[:-1]])
                c_base = (C.c_void_p * 4)(*[sbuf.data_ptr() + int(s) for s in starts])
            woffs, wtotal = _layout([w.size for w in want], MIS)
            wout = torch.full((wtotal,), CANARY, dtype=torch.uint8, device="cuda:0")
            w_dst = (C.c_void_p * 4)(*[wout.data_ptr() + x for x in woffs])
            torch.cuda.synchronize()
            assert L.zpk_codec_decode_batch_host_dptr_windows(codec.h, arc.ctypes.data, arc.size, dd.ctypes.data, 4, w_dst, res.ctypes.data, c_elem, c_base, None, wins.ctypes.data) == 0
            torch.cuda.synchronize()
            ps, ds, ws = codec.planes_stats(), codec.delta_stats(), codec.window_stats()
            assert (res["status"] == OK).all()
            _same(wout.cpu().numpy(), _want(wtotal, woffs, want), (variant, "host image"))
            # c.u8 has element size 1; with a base it would be staged for that anyway (delta_stats counts it), else only for its window
            assert ws["rows"] == 3 and ws["launches"] == 2 and ws["staged"] == (0 if bases else 1), (variant, ws)
            assert ds["staged"] == (1 if bases else 0) and ds["joined"] == (1 if bases else 0) and ps["joined"] == (1 if variant == "planes" else 0), (variant, ps, ds)
            assert ps["staged"] == 0
            wout.fill_(CANARY)
            torch.cuda.synchronize()
            assert L.zpk_codec_decode_batch_dimage_windows(codec.h, image_t.data_ptr(), image_t.numel(), dd.ctypes.data, 4, w_dst, 1, res.ctypes.data, c_elem, c_base, None, wins.ctypes.data) == 0
            torch.cuda.synchronize()
            assert (res["status"] == OK).all() and codec.window_stats() == dict(rows=3, launches=1, staged=0)      # (a device image decodes into the staging anyway)
            _same(wout.cpu().numpy(), _want(wtotal, woffs, want), (variant, "device image"))
    finally:
        codec.close()


# ------------------------------------------------------------------------------------------------ the torch view

def test_device_io_windows_end_to_end(torch, ckpt, tmp_path):
    new, old, raw = ckpt["new"], ckpt["old"], ckpt["raw"]
    path = tmp_path / "ckpt.zpk"
    path.write_bytes(ckpt["images"]["planes"])
    # the slice formula end to end: every dim of every tensor, from bytes, a file and a device image, beside entries read whole
    for archive in (ckpt["images"]["planes"], str(path), torch.from_numpy(np.frombuffer(ckpt["images"]["planes"], dtype=np.uint8).copy()).to("cuda:0")):
        for r in range(3):
            window = {k: (SHAPES[k], r, SHAPES[k][r] // 4, SHAPES[k][r] - SHAPES[k][r] // 3) for k in NAMES if r < len(SHAPES[k])}
            outs, status = device_io.read_files_device(archive, names=NAMES, planes="manifest", window=window)
            assert status == [OK] * 4
            for k, got in zip(NAMES, outs):
                t = new[k]
                if k in window:
                    _, dim, a, b = window[k]
                    t = t[(slice(None),) * dim + (slice(a, b),)]
                assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), _bytes(t)), (k, r)
    # negative dims; plain entries count bytes: shape in elements of size 1
    outs, status = device_io.read_files_device(ckpt["images"]["planes"], names=["b.fp32"], planes="manifest", window={"b.fp32": (SHAPES["b.fp32"], -1, 90, 96)})
    assert status == [OK] and np.array_equal(outs[0].cpu().numpy(), _bytes(new["b.fp32"][..., 90:96]))
    outs, status = device_io.read_files_device(ckpt["images"]["plain"], names=["a.bf16", "c.u8"], window={"a.bf16": ((128, 512), 1, 2, 6)})
    assert status == [OK, OK] and np.array_equal(outs[0].cpu().numpy(), raw["a.bf16"].reshape(128, 512)[:, 2:6].reshape(-1)) and np.array_equal(outs[1].cpu().numpy(), raw["c.u8"])
    # window=None and an empty dict are today's function
    a, sa = device_io.read_files_device(ckpt["images"]["planes"], planes="manifest")
    for w in (None, {}):
        b, sb = device_io.read_files_device(ckpt["images"]["planes"], planes="manifest", window=w)
        assert sa == sb and all(torch.equal(x, y) for x, y in zip(a, b))
    # with bases: the base is the window-size shard; in place it is the destination and what is returned
    window = {"a.bf16": (SHAPES["a.bf16"], 1, 32, 64), "b.fp32": (SHAPES["b.fp32"], 0, 1, 3), "c.u8": (SHAPES["c.u8"], 2, 512, 1024), "d.bf16": (SHAPES["d.bf16"], 1, 39, 40)}

    def cut(t, k):
        _, dim, a, b = window[k]
        return t[(slice(None),) * dim + (slice(a, b),)].contiguous()

    image = ckpt["images"]["delta"]
    shards = {k: cut(old[k], k) for k in NAMES}
    outs, status = device_io.read_files_device(image, planes="manifest", base=shards, window=window)
    assert status == [OK] * 4 and all(np.array_equal(got.cpu().numpy(), _bytes(cut(new[k], k))) for k, got in zip(NAMES, outs))
    assert all(torch.equal(shards[k], cut(old[k], k)) for k in NAMES)                   # the bases are only read
    outs, status = device_io.read_files_device(image, planes="manifest", base=shards, window=window, inplace=True)
    assert status == [OK] * 4 and all(outs[i] is shards[k] and torch.equal(shards[k], cut(new[k], k)) for i, k in enumerate(NAMES))
    with pytest.raises(ValueError, match="a.bf16"):                                     # a whole base is no shard
        device_io.read_files_device(image, planes="manifest", base=dict(shards, **{"a.bf16": old["a.bf16"]}), window=window)
    # a manifest that records base_xxh3: the hash of the WHOLE base, which the reader of a window does not hold
    checked = device_io.write_files_device(None, new, method=METHOD_LZ4, level=0, planes="dtype", base=old, check_base=True)
    shards = {k: cut(old[k], k) for k in NAMES}
    with pytest.raises(ValueError, match="WHOLE base"):
        device_io.read_files_device(checked, planes="manifest", base=shards, window=window)
    outs, status = device_io.read_files_device(checked, planes="manifest", base=shards, window=window, check_base=False)
    assert status == [OK] * 4 and all(np.array_equal(got.cpu().numpy(), _bytes(cut(new[k], k))) for k, got in zip(NAMES, outs))
    # ... entries read whole beside it are checked as ever
    outs, status = device_io.read_files_device(checked, names=["a.bf16", "c.u8"], planes="manifest", base={"a.bf16": old["a.bf16"].clone() + 1, "c.u8": old["c.u8"]})
    assert status == [BASE_MISMATCH, OK]
    # the ValueErrors, each naming its entry, before anything is decoded
    P = ckpt["images"]["planes"]
    for bad in (((128, 255), 0, 0, 1), ((128, 256), 2, 0, 1), ((128, 256), -3, 0, 1), ((128, 256), 1, 5, 4), ((128, 256), 1, 0, 257), ((128, 256), 0, -1, 4),
                ((), 0, 0, 0), ((128, 256), 0, 1)):
        with pytest.raises(ValueError, match="a.bf16"):
            device_io.read_files_device(P, names=["a.bf16"], planes="manifest", window={"a.bf16": bad})
    with pytest.raises(ValueError, match="a.bf16"):                                     # without planes the entry's elements are bytes
        device_io.read_files_device(P, names=["a.bf16"], window={"a.bf16": ((128, 256), 0, 0, 1)})
    with pytest.raises(KeyError, match="nope"):
        device_io.read_files_device(P, names=["a.bf16"], planes="manifest", window={"nope": ((1,), 0, 0, 1)})
