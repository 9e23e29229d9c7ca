"""Read-ahead for per-entry callers: zpack_read_file in CDR order is served from batches the context decodes ahead
(zpack_amd/host/readahead.c).  Every observable result — return code, every byte of the caller's buffer, reader.last_return —
must be the one the per-call path gives; the counters of include/zpack_amd.h show which path answered."""
import ctypes as C
import json
import math
import os
import threading

import numpy as np
import pytest

import zpack_amd
from benchdata import datagen as dg
from tests import zpk
from tests._libs import ZPackAPI, Reader, Stream, FileEntry, u8p, have_ref, ref, METHOD_NONE, METHOD_ZSTD, METHOD_LZ4

pytestmark = pytest.mark.gpu

KIB, MIB = 1 << 10, 1 << 20
FIRST_WINDOW = 512 * KIB          # the smallest a first window can be in bytes here (8 entries of 64 KiB)


@pytest.fixture(scope="module")
def Z():
    z = ZPackAPI(zpack_amd.ZPACK_SO)
    L = z.lib
    L.zpack_amd_read_ahead_stats.argtypes = [C.POINTER(Reader), C.c_void_p, C.POINTER(C.c_uint64)]
    L.zpack_create_dctx.restype = C.c_void_p
    L.zpack_create_dctx.argtypes = [C.c_int]
    L.zpack_free_dctx.restype = None
    L.zpack_free_dctx.argtypes = [C.c_int, C.c_void_p]
    L.zpack_reset_reader_dctx.restype = None
    L.zpack_reset_reader_dctx.argtypes = [C.POINTER(Reader)]
    L.zpack_read_files.argtypes = [C.POINTER(Reader), C.POINTER(C.POINTER(FileEntry)), C.c_uint64, C.POINTER(u8p),
                                   C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.c_void_p]
    return z


def _stats(Z, r, dctx=None):
    out = (C.c_uint64 * 6)()
    assert Z.lib.zpack_amd_read_ahead_stats(C.byref(r) if r is not None else None, dctx, out) == 0
    return dict(zip(("served", "own", "windows", "unused", "held", "cap"), (int(x) for x in out)))


def _dctx(Z, monkeypatch, setting):
    """an explicit context created under ZPACK_AMD_READ_AHEAD=setting (None: the default)"""
    if setting is None:
        monkeypatch.delenv("ZPACK_AMD_READ_AHEAD", raising=False)
    else:
        monkeypatch.setenv("ZPACK_AMD_READ_AHEAD", str(setting))
    x = Z.lib.zpack_create_dctx(METHOD_LZ4)
    monkeypatch.delenv("ZPACK_AMD_READ_AHEAD", raising=False)
    assert x
    return C.c_void_p(x)


def _read(Z, r, i, max_size, dctx=None, fill=None):
    out = (C.c_uint8 * max(1, max_size))()
    if fill is not None:
        C.memmove(out, fill, max(1, max_size))
    rc = Z.lib.zpack_read_file(C.byref(r), C.byref(r.file_entries[i]), C.cast(out, u8p), max_size, dctx)
    return rc, bytes(out[:max_size])


def _open_memory(Z, arc):
    r = Reader()
    keep = (C.c_uint8 * len(arc)).from_buffer_copy(arc)
    assert Z.lib.zpack_init_reader_memory_shared(C.byref(r), C.cast(keep, u8p), len(arc)) == 0
    return r, keep


def test_in_order_loop_memory_backed_lz4(Z, monkeypatch):
    """tests/read_archive.c's loop (NULL dctx) over 3000 x 64 KiB LZ4 entries, under a 16 MiB cap: all but the first call come
    from windows, which grow from one small window to the cap and then stay there"""
    cap = 16 * MIB
    monkeypatch.setenv("ZPACK_AMD_READ_AHEAD", str(cap))
    n, size = 3000, 64 * KIB
    b = dg.Batch(n, size, method=dg.LZ4, level=0, seed=61)
    r, keep = _open_memory(Z, b.archive.tobytes())
    assert _stats(Z, r)["windows"] == 0                     # no context yet
    for i in range(n):
        rc, out = _read(Z, r, i, size)
        assert rc == 0 and out == b.plaintext(i).tobytes(), i
    st = _stats(Z, r)
    assert st["cap"] == cap
    assert st["served"] >= n - 16 and st["served"] + st["own"] == n, st
    ramp = math.ceil(math.log2(cap / FIRST_WINDOW)) + 1
    assert n * size // cap <= st["windows"] <= ramp + math.ceil(n * size / cap) + 1, st
    assert st["unused"] == 0 and 0 < st["held"] <= cap + 16 * KIB * 64, st
    Z.close_reader(r)


def test_in_order_loop_file_backed_zstd_with_a_large_entry(Z, monkeypatch, tmp_path):
    """zpack_init_reader on a path, Zstandard level 3, mixed sizes, one entry above a quarter of the cap: that one is decoded on
    its own (today's per-call route), the runs before and after it come from windows"""
    cap = 4 * MIB
    monkeypatch.setenv("ZPACK_AMD_READ_AHEAD", str(cap))
    rng = np.random.default_rng(5)
    sizes = [int(x) for x in rng.integers(1, 200 * KIB, 120)]
    big_at = 57
    sizes[big_at] = cap // 4 + 12345
    files = [("z%03d" % i, dg.fill(i % 4, 23, i, s).tobytes()) for i, s in enumerate(sizes)]
    arc = Z.write_archive(files, METHOD_ZSTD, 3)
    path = tmp_path / "mixed.zpk"
    path.write_bytes(arc)
    r = Reader()
    assert Z.lib.zpack_init_reader(C.byref(r), str(path).encode()) == 0
    for i, (name, data) in enumerate(files):
        before = _stats(Z, r) if i else None
        rc, out = _read(Z, r, i, len(data) + 100)
        assert rc == 0 and out[:len(data)] == data, (i, rc)
        if i == big_at:
            after = _stats(Z, r)
            assert after["own"] == before["own"] + 1 and after["served"] == before["served"], (before, after)
    st = _stats(Z, r)
    assert st["windows"] >= 2 and st["served"] >= len(files) - 4, st
    Z.close_reader(r)


def test_off_switch(Z, monkeypatch):
    monkeypatch.setenv("ZPACK_AMD_READ_AHEAD", "0")
    n, size = 300, 64 * KIB
    b = dg.Batch(n, size, method=dg.LZ4, level=0, seed=62)
    r, keep = _open_memory(Z, b.archive.tobytes())
    for i in range(n):
        rc, out = _read(Z, r, i, size)
        assert rc == 0 and out == b.plaintext(i).tobytes(), i
    st = _stats(Z, r)
    assert st["served"] == 0 and st["windows"] == 0 and st["own"] == n and st["cap"] == 0, st
    Z.close_reader(r)


def test_random_order_reads_nothing_ahead(Z):
    n, size = 400, 32 * KIB
    b = dg.Batch(n, size, method=dg.ZSTD, level=3, seed=63)
    r, keep = _open_memory(Z, b.archive.tobytes())
    rng = np.random.default_rng(1)
    while True:                                             # a permutation without a single in-order step
        order = [int(x) for x in rng.permutation(n)]
        if not any(q == p + 1 for p, q in zip(order, order[1:])):
            break
    for i in order:
        rc, out = _read(Z, r, i, size)
        assert rc == 0 and out == b.plaintext(i).tobytes(), i
    st = _stats(Z, r)
    assert st["windows"] == 0 and st["served"] == 0 and st["own"] == n, st
    Z.close_reader(r)


# ----------------------------------------------------------------------------- verdict parity

def _load(golden_dir, name):
    with open(os.path.join(golden_dir, name)) as fh:
        return json.load(fh)


def _good(k):
    plain = dg.fill(k % 4, 71, k, 3000 + 997 * (k % 5)).tobytes()
    method = (METHOD_LZ4, METHOD_ZSTD, METHOD_NONE)[k % 3]
    return plain, dg.compress(method, 3 if method == METHOD_ZSTD else 0, plain), method


def _interleaved_archive(cases):
    """cases: [(payload region, offset delta, comp_size, uncomp_size, hash, method, recorded rc, recorded max_size)] — each bad
    entry sits between two good ones, so that it falls inside a read-ahead window"""
    payloads, ents, meta = [], [], []
    pos = 10
    for k, (region, delta, cs, us, h, m, rc, ms) in enumerate(cases):
        plain, frame, method = _good(k)
        payloads.append(frame)
        ents.append(("g%d" % k, pos, len(frame), len(plain), dg.xxh3(plain), method))
        meta.append((0, len(plain)))
        pos += len(frame)
        payloads.append(region)
        ents.append(("b%d" % k, pos + delta, cs, us, h, m))
        meta.append((rc, ms))
        pos += len(region)
    plain, frame, method = _good(len(cases))
    payloads.append(frame)
    ents.append(("tail", pos, len(frame), len(plain), dg.xxh3(plain), method))
    meta.append((0, len(plain)))
    return zpk.assemble(payloads, ents), meta


def _foreign_cases(golden_dir):
    out = []
    for c in _load(golden_dir, "foreign_frames.json"):
        fr = bytes.fromhex(c["frame"])
        out.append((fr, 0, len(fr), c["uncomp_size"], c["hash"], c["method"], c["rc"], c["max_size"]))
    return out


def _status_cases(golden_dir):
    """the payloads of status_cases.json moved into a new archive: the bytes around each payload come along, so that a tampered
    comp_size or offset reads what it read in the archive the reference judged; the offset-guard cases (whose verdict is about
    the end of THAT archive) are left out"""
    sc = _load(golden_dir, "status_cases.json")
    out = []
    for c in sc["cases"]:
        if "offset" in c["tamper"] and c["label"].split(":")[1].startswith("offset"):
            continue
        a = bytearray(bytes.fromhex(sc["bases"][c["base"]]))
        for p, x in c["flips"]:
            a[p] ^= x
        e = zpk.parse(a)[c["index"]]
        t = {**e, **{{"comp_method": "method"}.get(k, k): v for k, v in c["tamper"].items()}}
        lo = e["offset"]
        hi = min(len(a) - 12, max(e["offset"] + e["comp_size"], t["offset"] + t["comp_size"]) + 16)
        out.append((bytes(a[lo:hi]), t["offset"] - lo, t["comp_size"], t["uncomp_size"], t["hash"], t["method"], c["rc"], c["max_size"]))
    return out


def _call(api, r, i, ms_ref, how, dctx=None):
    """one zpack_read_file; the caller's buffer holds a pattern (or zeros) before the call"""
    us = r.file_entries[i].uncomp_size
    ms = {"exact": us, "roomy": us + 4096, "recorded": ms_ref}[how]
    fill = bytes(max(1, ms)) if how == "recorded" else (bytes(range(7, 256, 3)) * (ms // 83 + 1))[:max(1, ms)]
    out = (C.c_uint8 * max(1, ms)).from_buffer_copy(fill)
    rc = api.lib.zpack_read_file(C.byref(r), C.byref(r.file_entries[i]), C.cast(out, u8p), ms, dctx)
    return rc, bytes(out[:ms]), int(r.last_return)


def _pass(api, r, meta, how, dctx=None):
    """every entry in CDR order"""
    return [_call(api, r, i, ms_ref, how, dctx) for i, (rc_ref, ms_ref) in enumerate(meta)]


def _ref_pass(arc, meta, how):
    """the compiled reference, a fresh reader for every entry: its decoder contexts keep the state a failed entry left them in
    (a good LZ4 entry behind some of the foreign frames fails there otherwise, also after zpack_reset_reader_dctx)"""
    R = ref()
    keep = (C.c_uint8 * len(arc)).from_buffer_copy(arc)
    got = []
    for i, (rc_ref, ms_ref) in enumerate(meta):
        rr = Reader()
        assert R.lib.zpack_init_reader_memory_shared(C.byref(rr), C.cast(keep, u8p), len(arc)) == 0
        got.append(_call(R, rr, i, ms_ref, how))
        R.lib.zpack_close_reader(C.byref(rr))
    return got


@pytest.mark.parametrize("source", ["foreign_frames", "status_cases"])
def test_verdict_parity_on_damaged_and_odd_entries(Z, monkeypatch, golden_dir, source):
    cases = _foreign_cases(golden_dir) if source == "foreign_frames" else _status_cases(golden_dir)
    arc, meta = _interleaved_archive(cases)
    on, off = _dctx(Z, monkeypatch, None), _dctx(Z, monkeypatch, 0)
    for how in ("exact", "roomy", "recorded"):
        r_on, k_on = _open_memory(Z, arc)
        r_off, k_off = _open_memory(Z, arc)
        a = _pass(Z, r_on, meta, how, on)
        b = _pass(Z, r_off, meta, how, off)
        for i, (x, y) in enumerate(zip(a, b)):
            assert x[0] == y[0], (source, how, i, x[0], y[0])
            assert x[1] == y[1], (source, how, i, "buffer")
            assert x[2] == y[2], (source, how, i, "last_return", x[2], y[2])
            if how == "recorded":
                assert x[0] == meta[i][0], (source, i, x[0], meta[i][0])
        if have_ref():
            c = _ref_pass(arc, meta, how)
            for i, (x, z) in enumerate(zip(a, c)):
                assert x[0] == z[0], (source, how, i, "reference", x[0], z[0])
                if z[0] == 0:
                    assert x[1][:r_on.file_entries[i].uncomp_size] == z[1][:r_on.file_entries[i].uncomp_size], (source, how, i)
        Z.close_reader(r_on)
        Z.close_reader(r_off)
    st_on, st_off = _stats(Z, None, on), _stats(Z, None, off)
    # windows were in place, and they held entries the per-call path answered (unused: decoded ahead, never served)
    assert st_on["windows"] > 0 and st_on["served"] > len(meta) // 2 and st_on["unused"] > 0, st_on
    assert st_off["served"] == 0 and st_off["windows"] == 0, st_off
    Z.lib.zpack_free_dctx(METHOD_LZ4, on)
    Z.lib.zpack_free_dctx(METHOD_LZ4, off)


# ----------------------------------------------------------------------------- invalidation

def test_no_window_of_a_closed_reader(Z, monkeypatch):
    """read part of archive A in order with an explicit dctx, close the reader, reopen the SAME Reader struct on B — the same CDR,
    entry k damaged — and go on in order: entry k gets B's damage verdict, not A's bytes"""
    n, size, k = 40, 20 * KIB, 12
    b = dg.Batch(n, size, method=dg.LZ4, level=0, seed=64)
    arc_a = b.archive.tobytes()
    ents = zpk.parse(arc_a)
    bad = bytearray(arc_a)
    bad[ents[k]["offset"] + ents[k]["comp_size"] // 2] ^= 0x5A
    arc_b = bytes(bad)
    on, off = _dctx(Z, monkeypatch, None), _dctx(Z, monkeypatch, 0)
    r = Reader()
    ka = (C.c_uint8 * len(arc_a)).from_buffer_copy(arc_a)
    assert Z.lib.zpack_init_reader_memory_shared(C.byref(r), C.cast(ka, u8p), len(arc_a)) == 0
    for i in range(k):
        rc, out = _read(Z, r, i, size, on)
        assert rc == 0 and out == b.plaintext(i).tobytes()
    assert _stats(Z, None, on)["windows"] >= 2              # windows [1, 9) and [9, 25): entry k was decoded from A
    Z.close_reader(r)
    kb = (C.c_uint8 * len(arc_b)).from_buffer_copy(arc_b)
    assert Z.lib.zpack_init_reader_memory_shared(C.byref(r), C.cast(kb, u8p), len(arc_b)) == 0
    r2, k2 = _open_memory(Z, arc_b)
    want = _read(Z, r2, k, size, off)
    assert want[0] != 0
    got = _read(Z, r, k, size, on)
    assert got == want and r.last_return == r2.last_return
    for i in range(k + 1, n):
        rc, out = _read(Z, r, i, size, on)
        assert rc == 0 and out == b.plaintext(i).tobytes()
    Z.close_reader(r)
    Z.close_reader(r2)
    Z.lib.zpack_free_dctx(METHOD_LZ4, on)
    Z.lib.zpack_free_dctx(METHOD_LZ4, off)


@pytest.mark.parametrize("delta", [-10, 10])
def test_entry_changed_between_calls(Z, monkeypatch, delta):
    n, size, k = 30, 16 * KIB, 5
    b = dg.Batch(n, size, method=dg.ZSTD, level=3, seed=65)
    arc = b.archive.tobytes()
    on, off = _dctx(Z, monkeypatch, None), _dctx(Z, monkeypatch, 0)
    r, keep = _open_memory(Z, arc)
    r2, keep2 = _open_memory(Z, arc)
    for i in range(k):
        assert _read(Z, r, i, size, on) == (0, b.plaintext(i).tobytes())
    assert _stats(Z, None, on)["windows"] == 1
    for rr in (r, r2):
        rr.file_entries[k].uncomp_size = size + delta
    fill = bytes(range(256)) * (size // 128)
    want = _read(Z, r2, k, 2 * size, off, fill)
    got = _read(Z, r, k, 2 * size, on, fill)
    assert got == want and r.last_return == r2.last_return and want[0] != 0
    for i in range(k + 1, n):
        assert _read(Z, r, i, size, on) == (0, b.plaintext(i).tobytes())
    Z.close_reader(r)
    Z.close_reader(r2)
    Z.lib.zpack_free_dctx(METHOD_LZ4, on)
    Z.lib.zpack_free_dctx(METHOD_LZ4, off)


def test_empty_entries_do_not_end_a_run(Z):
    """empty files (comp_size 0, answered before any decode) scattered through the CDR: one run from the second call to the end"""
    payloads, ents, plains = [], [], []
    pos = 10
    for k in range(300):
        if k % 5 == 3:
            ents.append(("e%d" % k, pos, 0, 0, dg.xxh3(b""), METHOD_LZ4))
            plains.append(b"")
            continue
        plain = dg.fill(k % 4, 81, k, 20000 + 37 * k).tobytes()
        frame = dg.compress(METHOD_LZ4, 0, plain)
        payloads.append(frame)
        ents.append(("f%d" % k, pos, len(frame), len(plain), dg.xxh3(plain), METHOD_LZ4))
        plains.append(plain)
        pos += len(frame)
    r, keep = _open_memory(Z, zpk.assemble(payloads, ents))
    for i, plain in enumerate(plains):
        rc, out = _read(Z, r, i, 40000)
        assert rc == 0 and out[:len(plain)] == plain, i
    st = _stats(Z, r)
    full = sum(1 for p in plains if p)
    assert st["served"] == full - 1 and st["own"] == 1, st
    assert st["windows"] <= 8 and st["unused"] == 0, st
    Z.close_reader(r)


def test_reset_free_and_close_drop_the_window(Z):
    n, size = 64, 32 * KIB
    b = dg.Batch(n, size, method=dg.LZ4, level=0, seed=66)
    r, keep = _open_memory(Z, b.archive.tobytes())
    x = C.c_void_p(Z.lib.zpack_create_dctx(METHOD_LZ4))          # an explicit context freed while it holds a window
    for i in range(20):
        assert _read(Z, r, i, size, x) == (0, b.plaintext(i).tobytes())
    st = _stats(Z, None, x)
    assert st["held"] > 0 and st["windows"] == 2, st
    Z.lib.zpack_free_dctx(METHOD_LZ4, x)
    for i in range(20):
        assert _read(Z, r, i, size) == (0, b.plaintext(i).tobytes())
    assert _stats(Z, r)["held"] > 0
    Z.lib.zpack_reset_reader_dctx(C.byref(r))
    st = _stats(Z, r)
    assert st["held"] == 0 and st["unused"] > 0, st
    for i in range(20, n):                                  # a fresh run: first call on its own, then windows again
        assert _read(Z, r, i, size) == (0, b.plaintext(i).tobytes())
    assert _stats(Z, r)["served"] >= n - 3
    Z.close_reader(r)                                           # the reader's own context, window included, goes with it
    assert not r.zstd_dctx and _stats(Z, r)["held"] == 0


# ----------------------------------------------------------------------------- threads and interleaving

def _loop(Z, r, b, idx, dctx, size, errors, tag):
    for i in idx:
        rc, out = _read(Z, r, i, size, dctx)
        if rc != 0 or out != b.plaintext(i).tobytes():
            errors.append((tag, i, rc))
            return


def test_threads_own_contexts_and_one_shared_context(Z):
    n, size = 600, 64 * KIB
    b = dg.Batch(n, size, method=dg.LZ4, level=0, seed=67)
    r, keep = _open_memory(Z, b.archive.tobytes())
    ctxs = [Z.lib.zpack_create_dctx(METHOD_LZ4) for _ in range(4)]
    assert all(ctxs)
    errors = []
    ths = [threading.Thread(target=_loop, args=(Z, r, b, range(n), C.c_void_p(ctxs[t]), size, errors, "own%d" % t)) for t in range(4)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errors, errors[:5]
    for c in ctxs:
        assert _stats(Z, None, C.c_void_p(c))["served"] >= n - 16
        Z.lib.zpack_free_dctx(METHOD_LZ4, c)
    # two threads, one reader, NULL dctx: the reader's one context, disjoint halves in order
    ths = [threading.Thread(target=_loop, args=(Z, r, b, range(h * n // 2, (h + 1) * n // 2), None, size, errors, "half%d" % h))
           for h in range(2)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errors, errors[:5]
    st = _stats(Z, r)
    assert st["served"] + st["own"] == n, st
    Z.close_reader(r)


def _stream_entry(Z, r, i, dctx):
    e = r.file_entries[i]
    st = Stream()
    assert Z.lib.zpack_init_stream(C.byref(st)) == 0
    in_size, out_size = 4096, 8192
    in_buf = (C.c_uint8 * in_size)()
    out = (C.c_uint8 * max(1, e.uncomp_size))()
    st.next_out = C.cast(out, u8p)
    for _ in range(100000):
        if st.read_back:
            tail = C.string_at(C.addressof(st.next_in.contents) - st.read_back, st.read_back)
            C.memmove(in_buf, tail, st.read_back)
        st.next_in = C.cast(in_buf, u8p)
        st.avail_in = in_size
        st.avail_out = min(out_size, e.uncomp_size - st.total_out) or 1
        rc = Z.lib.zpack_read_file_stream(C.byref(r), C.byref(e), C.byref(st), dctx)
        assert rc == 0, rc
        if st.total_in == e.comp_size and st.read_back == 0:
            break
    Z.lib.zpack_close_stream(C.byref(st))
    return bytes(out[:st.total_out])


@pytest.mark.parametrize("explicit", [False, True])
def test_interleaved_batch_and_stream_reads(Z, explicit):
    n, size = 200, 48 * KIB
    b = dg.Batch(n, size, method=dg.ZSTD, level=3, seed=68)
    r, keep = _open_memory(Z, b.archive.tobytes())
    dctx = C.c_void_p(Z.lib.zpack_create_dctx(METHOD_ZSTD)) if explicit else None
    outs = [(C.c_uint8 * size)() for _ in range(3)]
    for i in range(n):
        assert _read(Z, r, i, size, dctx) == (0, b.plaintext(i).tobytes()), i
        if i % 17 == 5:
            pick = [(i * 31 + 7 * k) % n for k in range(3)]
            ents = (C.POINTER(FileEntry) * 3)(*[C.pointer(r.file_entries[j]) for j in pick])
            bufs = (u8p * 3)(*[C.cast(o, u8p) for o in outs])
            caps = (C.c_size_t * 3)(*([size] * 3))
            res = (C.c_int * 3)()
            assert Z.lib.zpack_read_files(C.byref(r), ents, 3, bufs, caps, res, dctx) == 0 and list(res) == [0, 0, 0]
            for j, o in zip(pick, outs):
                assert bytes(o) == b.plaintext(j).tobytes()
        if i % 23 == 11:
            j = (i * 13 + 3) % n
            assert _stream_entry(Z, r, j, dctx) == b.plaintext(j).tobytes(), j
    st = _stats(Z, r, dctx)
    assert st["served"] >= n - 16, st
    if explicit:
        Z.lib.zpack_free_dctx(METHOD_ZSTD, dctx)
    Z.close_reader(r)
