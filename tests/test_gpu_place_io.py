"""GPU: placed reads through the library (include/zpack_amd.h: zpack_amd_read_files_device_placed), the codec calls behind it and the
torch view (zpack_amd/device_io.py: read_files_device(..., place=)).

The archive holds COLUMN SHARDS, written with write_archive_device: weights of uint8, bf16 and fp32 as four shards of 8 x 96 elements
each, one bf16 weight whose first shard has rows of 8200 bytes (its 16 KiB items end mid-row), one whose first shard is the 320 KiB
frame the window tests use (block-parallel on a reader in host memory) and one of 640 KiB — stored, LZ4 and Zstandard, with and without
byte planes.  ONE placed read merges every weight on a memory reader, a file reader and a device-image reader; the reference is the
concatenate of what the _windows call (no windows: the entries whole) delivers for the same entries, and every byte of the destination
buffer outside the merged weights is a canary.

Then: window and placement together (a TP 3 -> TP 2 re-layout), delta entries in place over the merged previous checkpoint, a damaged
shard, too small a buffer, the refusals, dst_pitches == NULL against the _windows call, the sub-batch cut, and the torch view."""
import ctypes as C

import numpy as np
import pytest

import zpack_amd
from zpack_amd import device_io
from tests import zpk
from tests._libs import Reader, FileEntry, u8p, METHOD_NONE, METHOD_ZSTD, METHOD_LZ4
from tests.device_mem import torch, Z, _layout, CANARY, GAP            # noqa: F401  (torch, Z: fixtures)

pytestmark = pytest.mark.gpu

PFE = C.POINTER(FileEntry)
OK, BUFFER_TOO_SMALL, STREAM_INVALID = 0, 12, 21
MIS = (0, 1, 7, 15)
# weight: (torch dtype name, element size, rows, the shards' widths in elements)
WEIGHTS = {"u8": ("uint8", 1, 8, (96, 96, 96, 96)), "bf": ("bfloat16", 2, 8, (96, 96, 96, 96)), "f32": ("float32", 4, 8, (96, 96, 96, 96)),
           "mid": ("bfloat16", 2, 8, (4100, 96)), "frame": ("uint8", 1, 5, (65536, 1024)), "wide": ("uint8", 1, 5, (131072, 64))}
SHARDS = [(w, r) for w, spec in WEIGHTS.items() for r in range(len(spec[3]))]
NAMES = ["%s.tp%d" % s for s in SHARDS]
METHODS = {"stored": METHOD_NONE, "lz4": METHOD_LZ4, "zstd": METHOD_ZSTD}
VARIANTS = [(m, p) for m in METHODS for p in (False, True)]
WHERE = ["memory", "file", "device"]


class Window(C.Structure):
    _fields_ = [("row_bytes", C.c_uint64), ("row0", C.c_uint64), ("rows", C.c_uint64), ("col0", C.c_uint64), ("cols", C.c_uint64)]


@pytest.fixture(scope="module")
def P(Z):
    L = Z.lib
    R, vp, u64 = C.POINTER(Reader), C.c_void_p, C.c_uint64
    L.zpack_amd_read_files_device_placed.argtypes = [R, C.POINTER(PFE), u64, vp, C.POINTER(C.c_size_t), C.POINTER(C.c_uint8), C.POINTER(vp), C.POINTER(u64),
                                                     C.POINTER(Window), C.POINTER(u64), C.POINTER(C.c_int), vp]
    L.zpack_amd_read_files_device_windows.argtypes = [R, C.POINTER(PFE), u64, vp, C.POINTER(C.c_size_t), C.POINTER(C.c_uint8), C.POINTER(vp), C.POINTER(u64),
                                                      C.POINTER(Window), C.POINTER(C.c_int), vp]
    L.zpack_init_reader.argtypes = [R, C.c_char_p]
    return Z


def _bytes(t):
    return t.contiguous().view(-1).view(dtype=device_io._u8()).cpu().numpy().copy()


def _geometry(w):
    """(element size, rows, [(column offset, cols)] in bytes per shard, pitch in bytes) of weight w"""
    _, k, rows, widths = WEIGHTS[w]
    at, cols = 0, []
    for wd in widths:
        cols.append((at, wd * k))
        at += wd * k
    return k, rows, cols, at


@pytest.fixture(scope="module")
def ckpt(torch):
    """the weights (`new`) and the previous checkpoint (`old`), their shards, and the archives: (method, planes) -> bytes; "delta": LZ4,
    planes, each shard against its shard of `old`"""
    g = torch.Generator().manual_seed(38)
    new = {}
    for w, (dt, k, rows, widths) in WEIGHTS.items():
        cols = sum(widths)
        if dt == "uint8":
            new[w] = ((torch.arange(rows * cols, dtype=torch.int64) * 7 // 13 + len(new)) % 251).to(torch.uint8).reshape(rows, cols).to("cuda:0")
        else:
            new[w] = (torch.randn((rows, cols), generator=g) * 0.02).to(getattr(torch, dt)).to("cuda:0")
    old = {}
    for w, t in new.items():
        if t.dtype == torch.uint8:
            old[w] = t ^ 3
        else:
            old[w] = t.clone()
            flat = old[w].view(-1)
            flat[::16] = (flat[::16].float() * 1.01).to(flat.dtype)

    def shards(full):
        out = {}
        for w, r in SHARDS:
            widths = WEIGHTS[w][3]
            a = sum(widths[:r])
            out["%s.tp%d" % (w, r)] = full[w][:, a:a + widths[r]].contiguous()
        return out

    new_s, old_s = shards(new), shards(old)
    torch.cuda.synchronize()
    images = {}
    for m, planes in VARIANTS:
        images[(m, planes)] = bytes(_bytes(device_io.write_archive_device(new_s, method=METHODS[m], level=1 if m == "zstd" else 0, planes="dtype" if planes else None)))
    images["delta"] = bytes(_bytes(device_io.write_archive_device(new_s, method=METHOD_LZ4, level=0, planes="dtype", base=old_s)))
    for image in images.values():
        assert [e["filename"] for e in zpk.parse(image)[:len(NAMES)]] == NAMES
    return dict(new=new, old=old, new_s=new_s, old_s=old_s, raw={w: _bytes(t) for w, t in new.items()}, old_raw={w: _bytes(t) for w, t in old.items()}, images=images)


class Opened:
    """a reader over the image: in host memory, a file, or in device memory; ents: the shards' entries"""
    def __init__(self, P, torch, image, where, tmp_path=None):
        self.L, self.r = P.lib, Reader()
        if where == "memory":
            self.keep = (C.c_uint8 * len(image)).from_buffer_copy(image)
            assert self.L.zpack_init_reader_memory_shared(C.byref(self.r), C.cast(self.keep, u8p), len(image)) == 0
        elif where == "file":
            path = tmp_path / "p.zpk"
            path.write_bytes(image)
            assert self.L.zpack_init_reader(C.byref(self.r), str(path).encode()) == 0
        else:
            self.keep = torch.from_numpy(np.frombuffer(image, dtype=np.uint8).copy()).to("cuda:0")
            torch.cuda.synchronize()
            assert self.L.zpack_amd_init_reader_device(C.byref(self.r), self.keep.data_ptr(), len(image)) == 0
        self.ents = [self.r.file_entries[i] for i in range(len(NAMES))]

    def close(self):
        self.L.zpack_close_reader(C.byref(self.r))


def _elem(planes):
    return [WEIGHTS[w][1] for w, _ in SHARDS] if planes else None


def _raw_call(P, o, ents, addrs, caps, elem, bases, hashes, wins, pitches, call="placed"):
    n = len(ents)
    ptrs = (PFE * n)(*[C.pointer(e) for e in ents])
    res = (C.c_int * n)(*([-1] * n))
    c_elem = None if elem is None else (C.c_uint8 * n)(*elem)
    c_bases = None if bases is None else (C.c_void_p * n)(*bases)
    c_hash = None if hashes is None else (C.c_uint64 * n)(*hashes)
    c_win = None if wins is None else (Window * n)(*[Window(*w) for w in wins])
    args = [C.byref(o.r), ptrs, n, (C.c_void_p * n)(*addrs), (C.c_size_t * n)(*caps), c_elem, c_bases, c_hash, c_win]
    if call == "placed":
        rc = P.lib.zpack_amd_read_files_device_placed(*args, None if pitches is None else (C.c_uint64 * n)(*pitches), res, None)
    else:
        assert pitches is None
        rc = P.lib.zpack_amd_read_files_device_windows(*args, res, None)
    return rc, list(res), int(o.r.last_return)


def _merged_layout(weights=WEIGHTS):
    """every weight's merged matrix in one buffer between canaries -> ({weight: offset}, total)"""
    names = list(weights)
    offs, total = _layout([_geometry(w)[1] * _geometry(w)[3] for w in names], MIS)
    return dict(zip(names, offs)), total


def _placement(shards, at, base_addr):
    """addresses, max_sizes (the extents), windows and pitches of the shards, each entry whole, in merged buffers at base_addr + at[w]"""
    addrs, caps, wins, pitches = [], [], [], []
    for w, r in shards:
        k, rows, cols, pitch = _geometry(w)
        c0, cb = cols[r]
        addrs.append(base_addr + at[w] + c0)
        caps.append((rows - 1) * pitch + cb)
        wins.append((cb, 0, rows, 0, cb))
        pitches.append(pitch)
    return addrs, caps, wins, pitches


def _whole_read(P, torch, o, planes, bases=None):
    """the _windows call, no windows, every shard into a buffer of its own -> the shards' bytes, the results"""
    sizes = [int(e.uncomp_size) for e in o.ents]
    offs, total = _layout(sizes, MIS)
    buf = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda:0")
    c_b = None
    if bases is not None:
        bt = [torch.from_numpy(b).to("cuda:0") for b in bases]
        c_b = [t.data_ptr() for t in bt]
    torch.cuda.synchronize()
    head = _raw_call(P, o, o.ents, [buf.data_ptr() + x for x in offs], sizes, _elem(planes), c_b, None, None, None, call="windows")
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    return [h[x:x + s] for x, s in zip(offs, sizes)], head


def _concat(parts):
    """the shards' bytes, in SHARDS order -> {weight: the bytes of numpy's concatenate along the columns}"""
    out = {}
    for w in WEIGHTS:
        k, rows, cols, pitch = _geometry(w)
        out[w] = np.concatenate([parts[NAMES.index("%s.tp%d" % (w, r))].reshape(rows, cb) for r, (_, cb) in enumerate(cols)], axis=1).reshape(-1)
    return out


def _want(total, at, merged):
    w = np.full(total, CANARY, dtype=np.uint8)
    for name, x in at.items():
        if merged.get(name) is not None:
            w[x:x + merged[name].size] = merged[name]
    return w


def _same(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, int(bad[0]), bad.size)


# ------------------------------------------------------------------------------------------------ the merge

@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("variant", VARIANTS, ids=["%s-%s" % (m, "planes" if p else "plain") for m, p in VARIANTS])
def test_one_placed_read_merges_every_weight_as_the_concatenate_of_the_whole_reads(P, torch, ckpt, tmp_path, variant, where):
    planes = variant[1]
    o = Opened(P, torch, ckpt["images"][variant], where, tmp_path)
    try:
        parts, head = _whole_read(P, torch, o, planes)
        assert head == (OK, [OK] * len(NAMES), 0)
        merged = _concat(parts)
        for w in WEIGHTS:
            assert np.array_equal(merged[w], ckpt["raw"][w]), w                         # (... which is the weight)
        at, total = _merged_layout()
        buf = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda:0")
        addrs, caps, wins, pitches = _placement(SHARDS, at, buf.data_ptr())
        torch.cuda.synchronize()
        head = _raw_call(P, o, o.ents, addrs, caps, _elem(planes), None, None, wins, pitches)
        torch.cuda.synchronize()
        assert head == (OK, [OK] * len(NAMES), 0), head
        _same(buf.cpu().numpy(), _want(total, at, merged), variant)
        # a pick in another order beside entries that are not placed: the last shard of every weight placed, "u8.tp0" whole and dense
        pick = [NAMES.index("%s.tp%d" % (w, len(WEIGHTS[w][3]) - 1)) for w in reversed(list(WEIGHTS))] + [0]
        buf.fill_(CANARY)
        dense = torch.full((parts[0].size + 2 * GAP,), CANARY, dtype=torch.uint8, device="cuda:0")
        a2, c2, w2, p2 = _placement([SHARDS[i] for i in pick[:-1]], at, buf.data_ptr())
        torch.cuda.synchronize()
        head = _raw_call(P, o, [o.ents[i] for i in pick], a2 + [dense.data_ptr() + GAP], c2 + [parts[0].size], None if not planes else [_elem(True)[i] for i in pick], None, None,
                         w2 + [(0, 0, 0, 0, 0)], p2 + [0])
        torch.cuda.synchronize()
        assert head == (OK, [OK] * len(pick), 0), head
        want = np.full(total, CANARY, dtype=np.uint8)
        for i in pick[:-1]:
            w, r = SHARDS[i]
            k, rows, cols, pitch = _geometry(w)
            want[at[w]:at[w] + rows * pitch].reshape(rows, pitch)[:, cols[r][0]:cols[r][0] + cols[r][1]] = parts[i].reshape(rows, cols[r][1])
        _same(buf.cpu().numpy(), want, (variant, "a pick"))
        d = dense.cpu().numpy()
        assert np.array_equal(d[GAP:-GAP], parts[0]) and (d[:GAP] == CANARY).all() and (d[-GAP:] == CANARY).all()
    finally:
        o.close()


@pytest.mark.parametrize("where", WHERE)
def test_a_window_and_a_placement_together_relayout_tp3_to_tp2(P, torch, tmp_path, where):
    """one 12 x 96 fp32 matrix written as three column shards of 32; each of the two destination shards of 48 columns is built from the
    windows of two entries side by side, both in ONE call (the middle entry is read twice, once per half)"""
    g = torch.Generator().manual_seed(381)
    full = torch.randn((12, 96), generator=g).to("cuda:0")
    names = ["m.tp0", "m.tp1", "m.tp2"]
    image = bytes(_bytes(device_io.write_archive_device({nm: full[:, 32 * r:32 * r + 32].contiguous() for r, nm in enumerate(names)}, method=METHOD_LZ4, level=0, planes="dtype")))
    o = Opened(P, torch, image, where, tmp_path)
    try:
        ents = [o.r.file_entries[i] for i in range(3)]
        offs, total = _layout([12 * 48 * 4] * 2, (7, 1))
        buf = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda:0")
        D0, D1 = buf.data_ptr() + offs[0], buf.data_ptr() + offs[1]
        pitch, rb = 48 * 4, 32 * 4
        #          entry    destination        window (row_bytes, row0, rows, col0, cols)
        plan = [(ents[0], D0,            (rb, 0, 12, 0, rb)),        # tp0 whole           -> columns [0, 32) of shard 0
                (ents[1], D0 + 32 * 4,   (rb, 0, 12, 0, 16 * 4)),    # tp1 columns [0, 16)  -> columns [32, 48) of shard 0
                (ents[1], D1,            (rb, 0, 12, 16 * 4, 16 * 4)),   # tp1 columns [16, 32) -> columns [0, 16) of shard 1
                (ents[2], D1 + 16 * 4,   (rb, 0, 12, 0, rb))]        # tp2 whole           -> columns [16, 48) of shard 1
        caps = [11 * pitch + w[4] for _, _, w in plan]
        torch.cuda.synchronize()
        head = _raw_call(P, o, [p[0] for p in plan], [p[1] for p in plan], caps, [4] * 4, None, None, [p[2] for p in plan], [pitch] * 4)
        torch.cuda.synchronize()
        assert head == (OK, [OK] * 4, 0), head
        _same(buf.cpu().numpy(), _want(total, {"s0": offs[0], "s1": offs[1]}, {"s0": _bytes(full[:, :48]), "s1": _bytes(full[:, 48:])}), "tp3 -> tp2")
    finally:
        o.close()
    # the torch view: one read per destination shard
    d0, d1 = (torch.full((12, 48), 7.0, device="cuda:0") for _ in range(2))
    _, st = device_io.read_files_device(image, names=names[:2], planes="manifest", window={"m.tp1": ((12, 32), 1, 0, 16)}, place={"m.tp0": (d0, 1, 0), "m.tp1": (d0, 1, 32)})
    assert st == [OK, OK] and torch.equal(d0, full[:, :48])
    _, st = device_io.read_files_device(image, names=names[1:], planes="manifest", window={"m.tp1": ((12, 32), 1, 16, 32)}, place={"m.tp1": (d1, -1, 0), "m.tp2": (d1, -1, 16)})
    assert st == [OK, OK] and torch.equal(d1, full[:, 48:])


@pytest.mark.parametrize("where", WHERE)
def test_delta_entries_in_place_over_the_merged_previous_checkpoint(P, torch, ckpt, tmp_path, where):
    o = Opened(P, torch, ckpt["images"]["delta"], where, tmp_path)
    try:
        at, total = _merged_layout()
        prev = _want(total, at, ckpt["old_raw"])
        for inplace in (True, False):
            buf = torch.from_numpy(prev if inplace else np.full(total, CANARY, dtype=np.uint8)).to("cuda:0")
            bbuf = buf if inplace else torch.from_numpy(prev).to("cuda:0")
            addrs, caps, wins, pitches = _placement(SHARDS, at, buf.data_ptr())
            bases = [a - buf.data_ptr() + bbuf.data_ptr() for a in addrs]             # the same bytes of the merged previous checkpoint
            torch.cuda.synchronize()
            head = _raw_call(P, o, o.ents, addrs, caps, _elem(True), bases, None, wins, pitches)
            torch.cuda.synchronize()
            assert head == (OK, [OK] * len(NAMES), 0), head
            _same(buf.cpu().numpy(), _want(total, at, ckpt["raw"]), ("delta", inplace))
            if not inplace:
                assert np.array_equal(bbuf.cpu().numpy(), prev)                         # a base elsewhere is only read
    finally:
        o.close()


# ------------------------------------------------------------------------------------------------ verdicts

@pytest.mark.parametrize("where", WHERE)
def test_a_damaged_shard_leaves_its_sub_block_and_its_neighbours_are_delivered(P, torch, ckpt, tmp_path, where):
    image = ckpt["images"]["delta"]
    ents = zpk.parse(image)
    old_parts = [_bytes(ckpt["old_s"][nm]) for nm in NAMES]
    for j in (NAMES.index("bf.tp1"), NAMES.index("frame.tp0")):                         # a one-wave entry and the block-parallel one
        bad = bytearray(image); bad[ents[j]["offset"]] ^= 0xFF                          # the frame's first byte: no frame any more
        o = Opened(P, torch, bytes(bad), where, tmp_path)
        try:
            parts, headw = _whole_read(P, torch, o, True, bases=old_parts)
            assert headw[0] == OK and headw[1][j] != OK and all(v == OK for i, v in enumerate(headw[1]) if i != j), headw
            assert (parts[j] == CANARY).all()                                           # (the _windows call delivered nothing of it)
            at, total = _merged_layout()
            prev = _want(total, at, ckpt["old_raw"])
            w, r = SHARDS[j]
            k, rows, cols, pitch = _geometry(w)
            for inplace in (False, True):
                buf = torch.from_numpy(prev if inplace else np.full(total, CANARY, dtype=np.uint8)).to("cuda:0")
                bbuf = buf if inplace else torch.from_numpy(prev).to("cuda:0")
                addrs, caps, wins, pitches = _placement(SHARDS, at, buf.data_ptr())
                torch.cuda.synchronize()
                head = _raw_call(P, o, o.ents, addrs, caps, _elem(True), [a - buf.data_ptr() + bbuf.data_ptr() for a in addrs], None, wins, pitches)
                torch.cuda.synchronize()
                assert head == headw, (head, headw)                                     # results, return value and last_return: the _windows call's
                want = _want(total, at, ckpt["raw"])
                block = want[at[w]:at[w] + rows * pitch].reshape(rows, pitch)[:, cols[r][0]:cols[r][0] + cols[r][1]]
                block[:] = prev[at[w]:at[w] + rows * pitch].reshape(rows, pitch)[:, cols[r][0]:cols[r][0] + cols[r][1]] if inplace else CANARY
                _same(buf.cpu().numpy(), want, (NAMES[j], inplace))
        finally:
            o.close()


@pytest.mark.parametrize("where", WHERE)
def test_too_small_a_buffer_and_the_refusals(P, torch, ckpt, tmp_path, where):
    o = Opened(P, torch, ckpt["images"]["delta"], where, tmp_path)
    try:
        at, total = _merged_layout()
        prev = _want(total, at, ckpt["old_raw"])
        buf = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda:0")
        bbuf = torch.from_numpy(prev).to("cuda:0")
        addrs, caps, wins, pitches = _placement(SHARDS, at, buf.data_ptr())
        bases = [a - buf.data_ptr() + bbuf.data_ptr() for a in addrs]
        elem = _elem(True)
        merged = ckpt["raw"]
        # max_sizes[i] = extent - 1: BUFFER_TOO_SMALL for that entry alone, nothing of it written — though its window's bytes alone would fit
        for j in (NAMES.index("f32.tp2"), NAMES.index("frame.tp0")):
            room = list(caps); room[j] -= 1
            buf.fill_(CANARY)
            torch.cuda.synchronize()
            head = _raw_call(P, o, o.ents, addrs, room, elem, bases, None, wins, pitches)
            torch.cuda.synchronize()
            assert head[0] == OK and head[1] == [BUFFER_TOO_SMALL if i == j else OK for i in range(len(NAMES))], head
            want = _want(total, at, merged)
            w, r = SHARDS[j]
            k, rows, cols, pitch = _geometry(w)
            want[at[w]:at[w] + rows * pitch].reshape(rows, pitch)[:, cols[r][0]:cols[r][0] + cols[r][1]] = CANARY
            _same(buf.cpu().numpy(), want, ("too small", NAMES[j]))
        # invalid arguments: STREAM_INVALID, nothing moved, no result set
        buf.fill_(CANARY)
        torch.cuda.synchronize()
        j = NAMES.index("bf.tp1")
        cb = wins[j][4]

        def refused(what, **kw):
            a = dict(addrs=list(addrs), caps=list(caps), bases=list(bases), wins=list(wins), pitches=list(pitches), hashes=None)
            for key, (i, v) in kw.items():
                if key == "hashes":
                    a[key] = v
                else:
                    a[key][i] = v
            head = _raw_call(P, o, o.ents, a["addrs"], a["caps"], elem, a["bases"], a["hashes"], a["wins"], a["pitches"])
            assert head[0] == STREAM_INVALID and head[1] == [-1] * len(NAMES), (what, head)

        refused("a pitch below cols", pitches=(j, cb - 1))
        refused("a pitch below cols by a lot", pitches=(j, 1))
        refused("an extent that wraps", pitches=(j, 2 ** 64 // 7 + 1))
        refused("a pitch without a window", wins=(j, (0, 0, 0, 0, 0)))
        refused("a window that is none of the entry", wins=(j, (cb, 0, 9, 0, cb)))
        refused("a base overlapping by one byte", bases=(j, addrs[j] + caps[j] - 1))
        refused("a base one byte behind", bases=(j, addrs[j] + 1))
        refused("a base in the gaps", bases=(j, addrs[j] + cb))
        refused("a hash for a pitched base", hashes=(0, [0] * len(NAMES)))
        torch.cuda.synchronize()
        assert bool((buf == CANARY).all()) and np.array_equal(bbuf.cpu().numpy(), prev)
        # ... while a placed base whose extent IS its window's bytes (pitch == cols) is hashed and checked as ever
        one = NAMES.index("u8.tp3")
        k, rows, cols, pitch = _geometry("u8")
        n1 = rows * cols[3][1]
        shard_old = torch.from_numpy(_bytes(ckpt["old_s"]["u8.tp3"])).to("cuda:0")
        good = device_io.hash_tensors([shard_old])
        for hashes, status in ((good, OK), ([good[0] ^ 1], 64)):
            out = torch.full((n1 + 2 * GAP,), CANARY, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            head = _raw_call(P, o, [o.ents[one]], [out.data_ptr() + GAP], [n1], [1], [shard_old.data_ptr()], hashes, [(cols[3][1], 0, rows, 0, cols[3][1])], [cols[3][1]])
            torch.cuda.synchronize()
            assert head[:2] == (OK, [status]), head
            got = out.cpu().numpy()
            assert np.array_equal(got[GAP:-GAP], _bytes(ckpt["new_s"]["u8.tp3"]) if status == OK else np.full(n1, CANARY, dtype=np.uint8))
            assert (got[:GAP] == CANARY).all() and (got[-GAP:] == CANARY).all()
    finally:
        o.close()


# ------------------------------------------------------------------------------------------------ the codec: NULL pitches, sub-batches, counts

def _codec_protos():
    L = zpack_amd.lib()
    vp, u64 = C.c_void_p, C.c_uint64
    L.zpk_codec_decode_batch_host_dptr_windows.argtypes = [vp, vp, u64, vp, u64, vp, vp, vp, vp, vp, vp]
    L.zpk_codec_decode_batch_dimage_windows.argtypes = [vp, vp, u64, vp, u64, vp, C.c_int, vp, vp, vp, vp, vp]
    L.zpk_codec_decode_batch_host_dptr_placed.argtypes = [vp, vp, u64, vp, u64, vp, vp, vp, vp, vp, vp, vp]
    L.zpk_codec_decode_batch_dimage_placed.argtypes = [vp, vp, u64, vp, u64, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    return L


def _descs(image, caps):
    ents = zpk.parse(image)[:len(NAMES)]
    dd = np.zeros(len(NAMES), dtype=zpack_amd.DECODE_DESC)
    for i, e in enumerate(ents):
        dd[i] = (e["offset"], e["comp_size"], e["uncomp_size"], e["hash"], 0, caps[i], e["method"], 0)
    return dd


def test_null_pitches_are_the_windows_call_bytes_results_and_counts(torch, ckpt):
    L = _codec_protos()
    image = ckpt["images"][("lz4", True)]
    arc = np.frombuffer(image, dtype=np.uint8)
    image_t = torch.from_numpy(arc.copy()).to("cuda:0")
    n = len(NAMES)
    elem = (C.c_uint8 * n)(*_elem(True))
    # windows on half of the entries: their first row, densely
    wins = np.zeros(n, dtype=zpack_amd.WINDOW)
    caps = []
    for i, (w, r) in enumerate(SHARDS):
        k, rows, cols, pitch = _geometry(w)
        if i % 2:
            wins[i] = (cols[r][1], 1, 1, 0, cols[r][1])
        caps.append(cols[r][1] if i % 2 else rows * cols[r][1])
    dd = _descs(image, caps)
    offs, total = _layout(caps, MIS)
    codec = zpack_amd.Codec(0)
    try:
        outs = []
        for call in ("windows", "placed NULL", "placed zeros"):
            for dimage in (False, True):
                out = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda:0")
                c_dst = (C.c_void_p * n)(*[out.data_ptr() + x for x in offs])
                res = np.zeros(n, dtype=zpack_amd.DECODE_RESULT)
                zeros = np.zeros(n, dtype=np.uint64)
                tail = () if call == "windows" else (None,) if call == "placed NULL" else (zeros.ctypes.data,)
                torch.cuda.synchronize()
                if dimage:
                    f = L.zpk_codec_decode_batch_dimage_windows if call == "windows" else L.zpk_codec_decode_batch_dimage_placed
                    rc = f(codec.h, image_t.data_ptr(), image_t.numel(), dd.ctypes.data, n, c_dst, 1, res.ctypes.data, elem, None, None, wins.ctypes.data, *tail)
                else:
                    f = L.zpk_codec_decode_batch_host_dptr_windows if call == "windows" else L.zpk_codec_decode_batch_host_dptr_placed
                    rc = f(codec.h, arc.ctypes.data, arc.size, dd.ctypes.data, n, c_dst, res.ctypes.data, elem, None, None, wins.ctypes.data, *tail)
                torch.cuda.synchronize()
                assert rc == 0 and (res["status"] == OK).all()
                assert codec.place_stats() == dict(rows=0, launches=0)
                outs.append((dimage, out.cpu().numpy(), res.tobytes(), codec.window_stats(), codec.planes_stats(), codec.decode_stats()["span_copy_launches"]))
        for dimage in (False, True):
            mine = [x for x in outs if x[0] == dimage]
            assert mine[0][3]["rows"] == n // 2
            for other in mine[1:]:
                assert np.array_equal(other[1], mine[0][1]) and other[2:] == mine[0][2:]
    finally:
        codec.close()


def test_a_small_dimage_chunk_cuts_the_pitches_with_their_sub_batches(torch, ckpt):
    """the pitch column is cut (a device image) and gathered (an image in host memory: the large frames leave the batch, the rest is
    gathered behind them) with the other four"""
    L = _codec_protos()
    image = ckpt["images"][("lz4", True)]
    arc = np.frombuffer(image, dtype=np.uint8)
    image_t = torch.from_numpy(arc.copy()).to("cuda:0")
    n = len(NAMES)
    at, total = _merged_layout()
    out = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda:0")
    addrs, caps, wins, pitches = _placement(SHARDS, at, out.data_ptr())
    # every other entry of the small weights is NOT placed: pitch 0 beside its window is the _windows call's dense delivery, so it goes elsewhere
    dense = [i for i, (w, r) in enumerate(SHARDS) if w in ("u8", "bf", "f32") and r % 2]
    doffs, dtotal = _layout([8 * wins[i][4] for i in dense], MIS)
    dbuf = torch.full((dtotal,), CANARY, dtype=torch.uint8, device="cuda:0")
    for i, x in zip(dense, doffs):
        addrs[i], caps[i], pitches[i] = dbuf.data_ptr() + x, 8 * wins[i][4], 0
    dd = _descs(image, caps)
    c_dst = (C.c_void_p * n)(*addrs)
    elem = (C.c_uint8 * n)(*_elem(True))
    c_win = np.array(wins, dtype=zpack_amd.WINDOW)
    c_pitch = np.array(pitches, dtype=np.uint64)
    want = _want(total, at, ckpt["raw"])
    parts = {i: _bytes(ckpt["new_s"][NAMES[i]]) for i in dense}
    for i in dense:
        w, r = SHARDS[i]
        k, rows, cols, pitch = _geometry(w)
        want[at[w]:at[w] + rows * pitch].reshape(rows, pitch)[:, cols[r][0]:cols[r][0] + cols[r][1]] = CANARY
    dwant = _want(dtotal, dict(zip(dense, doffs)), parts)
    res = np.zeros(n, dtype=zpack_amd.DECODE_RESULT)
    codec = zpack_amd.Codec(0)
    try:
        seen = set()
        for chunk in (0, 700 << 10, 64 << 10):
            codec.set_option(zpack_amd.OPT_DIMAGE_CHUNK, chunk)
            out.fill_(CANARY); dbuf.fill_(CANARY)
            torch.cuda.synchronize()
            assert L.zpk_codec_decode_batch_dimage_placed(codec.h, image_t.data_ptr(), image_t.numel(), dd.ctypes.data, n, c_dst, 1, res.ctypes.data, elem, None, None,
                                                          c_win.ctypes.data, c_pitch.ctypes.data) == 0
            torch.cuda.synchronize()
            subs = codec.dimage_stats()["sub_batches"]
            seen.add(subs)
            assert (res["status"] == OK).all()
            ps, ws = codec.place_stats(), codec.window_stats()
            assert ps["rows"] == n - len(dense) and ws["rows"] == len(dense) and 1 <= ps["launches"] <= subs and 1 <= ws["launches"] <= subs, (chunk, subs, ps, ws)
            _same(out.cpu().numpy(), want, ("device image", chunk))
            _same(dbuf.cpu().numpy(), dwant, ("device image, dense", chunk))
        assert 1 in seen and max(seen) >= 4, seen                                       # one sub-batch, and many
        codec.set_option(zpack_amd.OPT_DIMAGE_CHUNK, 0)
        out.fill_(CANARY); dbuf.fill_(CANARY)
        torch.cuda.synchronize()
        assert L.zpk_codec_decode_batch_host_dptr_placed(codec.h, arc.ctypes.data, arc.size, dd.ctypes.data, n, c_dst, res.ctypes.data, elem, None, None,
                                                         c_win.ctypes.data, c_pitch.ctypes.data) == 0
        torch.cuda.synchronize()
        assert (res["status"] == OK).all()
        ps, ws = codec.place_stats(), codec.window_stats()
        assert ps["rows"] == n - len(dense) and ps["launches"] >= 2 and ws["rows"] == len(dense), (ps, ws)       # the large frames one by one, the rest gathered
        _same(out.cpu().numpy(), want, "host image")
        _same(dbuf.cpu().numpy(), dwant, "host image, dense")
        # host destinations take no pitch; a pitch takes a window
        hp = (C.c_void_p * n)(*[0x1000] * n)
        assert L.zpk_codec_decode_batch_dimage_placed(codec.h, image_t.data_ptr(), image_t.numel(), dd.ctypes.data, n, hp, 0, res.ctypes.data, None, None, None, None, c_pitch.ctypes.data) == -2
        assert L.zpk_codec_decode_batch_host_dptr_placed(codec.h, arc.ctypes.data, arc.size, dd.ctypes.data, n, c_dst, res.ctypes.data, elem, None, None, None, c_pitch.ctypes.data) == -2
        torch.cuda.synchronize()
    finally:
        codec.close()


# ------------------------------------------------------------------------------------------------ the torch view

def test_device_io_place_end_to_end(torch, ckpt, tmp_path):
    new, old = ckpt["new"], ckpt["old"]
    image = ckpt["images"][("zstd", True)]
    path = tmp_path / "ckpt.zpk"
    path.write_bytes(image)

    def places(dests):
        return {"%s.tp%d" % (w, r): (dests[w], 1, sum(WEIGHTS[w][3][:r])) for w, r in SHARDS}

    for archive in (image, str(path), torch.from_numpy(np.frombuffer(image, dtype=np.uint8).copy()).to("cuda:0")):
        dests = {w: torch.zeros_like(t) for w, t in new.items()}
        outs, status = device_io.read_files_device(archive, names=NAMES, planes="manifest", place=places(dests))
        assert status == [OK] * len(NAMES)
        assert all(outs[i] is dests[w] for i, (w, _) in enumerate(SHARDS)) and all(torch.equal(dests[w], new[w]) for w in WEIGHTS)
    # only some entries placed, beside entries read as ever; a 3-D destination, merged along its middle dimension
    dest3 = torch.zeros((2, 4 * 96, 4), dtype=torch.bfloat16, device="cuda:0")
    bf = ["bf.tp%d" % r for r in range(4)]
    outs, status = device_io.read_files_device(image, names=bf + ["u8.tp0"], planes="manifest", place={nm: (dest3, 1, 96 * r) for r, nm in enumerate(bf)})
    assert status == [OK] * 5 and np.array_equal(outs[4].cpu().numpy(), _bytes(ckpt["new_s"]["u8.tp0"]))
    want3 = torch.cat([ckpt["new_s"][nm].reshape(2, 96, 4) for nm in bf], dim=1)
    assert torch.equal(dest3, want3)
    # place=None and an empty dict are today's function
    a, sa = device_io.read_files_device(image, planes="manifest")
    for p in (None, {}):
        b, sb = device_io.read_files_device(image, planes="manifest", place=p)
        assert sa == sb and all(torch.equal(x, y) for x, y in zip(a, b))
    # delta entries: in place the destination is its own base; apart, the base is a tensor in the merged layout and is only read
    delta = ckpt["images"]["delta"]
    prev = {w: t.clone() for w, t in old.items()}
    outs, status = device_io.read_files_device(delta, names=NAMES, planes="manifest", base={nm: prev[w] for nm, (w, _) in zip(NAMES, SHARDS)}, inplace=True, place=places(prev))
    assert status == [OK] * len(NAMES) and all(torch.equal(prev[w], new[w]) for w in WEIGHTS)
    dests = {w: torch.zeros_like(t) for w, t in new.items()}
    outs, status = device_io.read_files_device(delta, names=NAMES, planes="manifest", base={nm: old[w] for nm, (w, _) in zip(NAMES, SHARDS)}, place=places(dests))
    assert status == [OK] * len(NAMES) and all(torch.equal(dests[w], new[w]) for w in WEIGHTS) and all(torch.equal(old[w], ckpt["old"][w]) for w in WEIGHTS)
    with pytest.raises(ValueError, match="bf.tp1"):                                     # in place the destination IS the base
        device_io.read_files_device(delta, names=["bf.tp1"], planes="manifest", base={"bf.tp1": old["bf"]}, inplace=True, place={"bf.tp1": (dests["bf"], 1, 96)})
    # a manifest that records base_xxh3: as a windowed entry is handled
    checked = device_io.write_archive_device(ckpt["new_s"], method=METHOD_LZ4, level=0, planes="dtype", base=ckpt["old_s"], check_base=True)
    prev = {w: t.clone() for w, t in old.items()}
    kw = dict(names=NAMES, planes="manifest", base={nm: prev[w] for nm, (w, _) in zip(NAMES, SHARDS)}, inplace=True, place=places(prev))
    with pytest.raises(ValueError, match="check_base=False"):
        device_io.read_files_device(checked, **kw)
    assert all(torch.equal(prev[w], old[w]) for w in WEIGHTS)
    outs, status = device_io.read_files_device(checked, check_base=False, **kw)
    assert status == [OK] * len(NAMES) and all(torch.equal(prev[w], new[w]) for w in WEIGHTS)
    # the ValueErrors, each naming its entry, before anything is decoded
    d = torch.zeros((8, 384), dtype=torch.bfloat16, device="cuda:0")
    for bad in ((torch.zeros((7, 384), dtype=torch.bfloat16, device="cuda:0"), 1, 0),   # a size that does not divide into 7 rows
                (d, 1, 289), (d, 1, -1), (d, 2, 0), (d, -3, 0),                         # a slice past the destination; a dim out of range
                (d.t(), 1, 0), (d.cpu(), 1, 0), (d,)):                                  # not contiguous; not on the device; not a triple
        with pytest.raises(ValueError, match="bf.tp1"):
            device_io.read_files_device(image, names=["bf.tp1"], planes="manifest", place={"bf.tp1": bad})
    assert not bool(d.any())
    with pytest.raises(ValueError, match="bf.tp1"):                                     # a window whose rows are not the destination's
        device_io.read_files_device(image, names=["bf.tp1"], planes="manifest", window={"bf.tp1": ((8, 96), 1, 0, 48)}, place={"bf.tp1": (torch.zeros((4, 192), dtype=torch.bfloat16, device="cuda:0"), 1, 0)})
    with pytest.raises(KeyError, match="nope"):
        device_io.read_files_device(image, names=["bf.tp1"], planes="manifest", place={"nope": (d, 1, 0)})
