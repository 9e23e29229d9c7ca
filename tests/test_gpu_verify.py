"""GPU: entries TESTED on the device — zpack_amd_test_files (include/zpack_amd.h), the codec calls behind it (zpk_codec_verify_batch_host,
zpk_codec_verify_batch_dimage, zpk_codec_verify_stats: include/zpack_codec.h), the hash-only kernel of stored entries (stored_hash.h) and
the torch view (device_io.test_files).

Every expectation comes from the existing read path, the oracle and the golden fixtures, none from the new code: results, return value
and last_return of a test call are those of zpack_read_files into ZERO-FILLED buffers of exactly uncomp_size bytes, through a memory
reader, a file reader and a reader over an image in device memory; the codec calls give the results of the codec's read calls field for
field and take the same routes; hashes are the oracle's XXH3.  Memory comes from torch."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import zpack_amd
from benchdata import datagen as dg
from tests import zpk
from tests._libs import Reader, FileEntry, u8p, oracle
from tests.device_mem import torch, Z, _plain, _build                                 # noqa: F401  (torch, Z: fixtures)

pytestmark = pytest.mark.gpu

PFE = C.POINTER(FileEntry)
KINDS = ("memory", "file", "device")
NOT_AVAILABLE = 24
SENTINEL = 0x5EED
ROUTES = ("frame_parallel_entries", "device_walked", "device_walk_accepted", "stored_span_entries", "stored_span_groups")    # decode_stats2 out[5], [10]..[13]


# ------------------------------------------------------------------------------------------------ helpers

@pytest.fixture(scope="module")
def ZT(Z):
    Z.lib.zpack_amd_test_files.argtypes = [C.POINTER(Reader), C.POINTER(PFE), C.c_uint64, C.POINTER(C.c_int), C.c_void_p]
    return Z


@pytest.fixture(scope="module")
def codec():
    c = zpack_amd.Codec(0)
    yield c
    c.close()


def _image(torch, arc, shift=0):
    t = torch.full((shift + len(arc) + 3,), 0xEE, dtype=torch.uint8, device="cuda:0")
    t[shift:shift + len(arc)] = torch.from_numpy(np.frombuffer(arc, dtype=np.uint8).copy())
    torch.cuda.synchronize()
    return t


def _open(Z, torch, kind, arc, tmp_path, shift=3):
    """-> (the reader, whatever has to stay alive with it)"""
    r = Reader()
    if kind == "memory":
        keep = (C.c_uint8 * len(arc)).from_buffer_copy(arc)
        assert Z.lib.zpack_init_reader_memory_shared(C.byref(r), C.cast(keep, u8p), len(arc)) == 0
    elif kind == "file":
        keep = os.path.join(str(tmp_path), "arc_%d.zpk" % len(os.listdir(str(tmp_path))))
        with open(keep, "wb") as fh:
            fh.write(arc)
        assert Z.lib.zpack_init_reader(C.byref(r), keep.encode()) == 0
    else:
        keep = _image(torch, arc, shift)
        assert Z.lib.zpack_amd_init_reader_device(C.byref(r), keep.data_ptr() + shift, len(arc)) == 0
    return r, keep


def _entries(r, picks=None, tamper=None):
    """copies of the reader's entries `picks` (None: all), entry k with the fields of tamper[k] changed"""
    picks = list(range(r.file_count)) if picks is None else picks
    out = []
    for k, i in enumerate(picks):
        e = FileEntry.from_buffer_copy(r.file_entries[i])
        for f, v in (tamper or {}).get(k, {}).items():
            setattr(e, {"method": "comp_method"}.get(f, f), v)
        out.append(e)
    return out


def _read(Z, r, ents, fill=0):
    """zpack_read_files into buffers of exactly uncomp_size bytes filled with `fill` -> (rc, results, last_return)"""
    n = len(ents)
    bufs = [np.full(max(1, int(e.uncomp_size)), fill, dtype=np.uint8) for e in ents]
    res = (C.c_int * max(n, 1))(*([-1] * max(n, 1)))
    r.last_return = SENTINEL
    rc = Z.lib.zpack_read_files(C.byref(r), (PFE * max(n, 1))(*[C.pointer(e) for e in ents]), n, (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs]),
                                (C.c_size_t * max(n, 1))(*[int(e.uncomp_size) for e in ents]), res, None)
    return rc, list(res)[:n], int(r.last_return)


def _test(Z, r, ents, dctx=None):
    """zpack_amd_test_files -> (rc, results, last_return)"""
    n = len(ents)
    res = (C.c_int * max(n, 1))(*([-1] * max(n, 1)))
    r.last_return = SENTINEL
    rc = Z.lib.zpack_amd_test_files(C.byref(r), (PFE * max(n, 1))(*[C.pointer(e) for e in ents]), n, res, dctx)
    return rc, list(res)[:n], int(r.last_return)


def _parity(Z, torch, tmp_path, arc, picks=None, tamper=None, kinds=KINDS):
    """the test call against the read into zero-filled exact-size buffers, through every kind of reader -> the memory reader's read"""
    first = None
    for kind in kinds:
        r, keep = _open(Z, torch, kind, arc, tmp_path)
        try:
            ents = _entries(r, picks, tamper)
            want = _read(Z, r, ents)
            got = _test(Z, r, ents)
            assert got == want, (kind, got, want)
            assert want[0] == 0 and -1 not in want[1]
            first = first or want
        finally:
            Z.lib.zpack_close_reader(C.byref(r))
    return first


def _desc_of(arc, tamper=None):
    pe = zpk.parse(arc)
    desc = np.zeros(len(pe), dtype=zpack_amd.DECODE_DESC)
    for k, (d, e) in enumerate(zip(desc, pe)):
        e = {**e, **(tamper or {}).get(k, {})}
        d["src_offset"], d["comp_size"], d["uncomp_size"], d["expect_hash"] = e["offset"], e["comp_size"], e["uncomp_size"], e["hash"]
        d["dst_capacity"], d["method"] = e["uncomp_size"], e["method"]
    return desc


def _codec_parity(codec, torch, arc, desc):
    """the codec's verify calls against its read calls (zero-filled exact-size host buffers): results field for field, the same routes
    -> (the results, the routes of the host call, the routes of the device-image call)"""
    image = _image(torch, arc, 5)[5:5 + len(arc)]
    res_r, outs = codec.decode_batch_host(arc, desc)
    st_r = codec.decode_stats()
    res_v = codec.verify_batch_host(arc, desc)
    st_v = codec.decode_stats()
    assert res_v.tobytes() == res_r.tobytes(), [(i, a, b) for i, (a, b) in enumerate(zip(res_v, res_r)) if a != b][:4]
    assert [st_v[k] for k in ROUTES] == [st_r[k] for k in ROUTES], (st_v, st_r)
    assert codec.verify_stats()["bytes_copied_home"] == 0
    dres_r, outs = codec.decode_batch_dimage(image, desc)
    dst_r = codec.decode_stats()
    dres_v = codec.verify_batch_dimage(image, desc)
    dst_v = codec.decode_stats()
    assert dres_v.tobytes() == dres_r.tobytes(), [(i, a, b) for i, (a, b) in enumerate(zip(dres_v, dres_r)) if a != b][:4]
    assert [dst_v[k] for k in ROUTES] == [dst_r[k] for k in ROUTES], (dst_v, dst_r)
    assert [int(x) for x in dres_r["status"]] == [int(x) for x in res_r["status"]]
    assert codec.verify_stats()["bytes_copied_home"] == 0 and codec.dimage_stats()["span_copy_launches"] == 0
    return res_v, st_v, dst_v


def _load(golden_dir, name):
    with open(os.path.join(golden_dir, name)) as fh:
        return json.load(fh)


# ------------------------------------------------------------------------------------------------ the synthetic archive

SIZES = [1, 240, 241, 1024, 0, 1025, 65536, 320 << 10, 3 << 19]                        # (the empty entries lie in the middle)
METHODS = [(dg.NONE, 0), (dg.LZ4, 0), (dg.ZSTD, 3)]


@pytest.fixture(scope="module")
def synth():
    """stored, LZ4 and Zstandard entries of every size in SIZES (text: the large compressed ones are worth a block-parallel turn)"""
    specs = [(m, lv, dg.fill(dg.TEXT, 31, 3 * si + mi, n).tobytes()) for si, n in enumerate(SIZES) for mi, (m, lv) in enumerate(METHODS)]
    return dict(arc=_build(specs), specs=specs)


def _index(size, method):
    return 3 * SIZES.index(size) + [m for m, _ in METHODS].index(method)


# ------------------------------------------------------------------------------------------------ 1. parity

@pytest.mark.parametrize("name", ["archive_none.zpk", "archive_zstd.zpk", "archive_lz4.zpk"])
def test_parity_on_the_reference_archives(ZT, torch, tmp_path, golden_dir, name):
    arc = open(os.path.join(golden_dir, "ref_workdir", name), "rb").read()
    assert _parity(ZT, torch, tmp_path, arc) == (0, [0, 0], 0)


def test_parity_on_every_status_case(ZT, torch, tmp_path, golden_dir):
    """every case of status_cases.json: the cases of one archive (a base with its flipped bytes) are one batch of tampered entries"""
    sc = _load(golden_dir, "status_cases.json")
    groups = {}
    for c in sc["cases"]:
        groups.setdefault((c["base"], tuple(tuple(f) for f in c["flips"])), []).append(c)
    seen, verdicts = 0, set()
    for (base, flips), cases in groups.items():
        a = bytearray(bytes.fromhex(sc["bases"][base]))
        for p, x in flips:
            a[p] ^= x
        picks = [c["index"] for c in cases]
        tamper = {k: c["tamper"] for k, c in enumerate(cases)}
        rc, res, last = _parity(ZT, torch, tmp_path, bytes(a), picks, tamper)
        for c, v in zip(cases, res):
            if c["max_size"] == {**zpk.parse(a)[c["index"]], **c["tamper"]}["uncomp_size"]:
                assert v == c["rc"], (c["label"], v, c["rc"])                          # the reference's recorded verdict, where its buffer was an exact one
            verdicts.add(v)
        seen += len(cases)
    assert seen == len(sc["cases"]) == 82 and {0, 13, 15, 16, 18, 19} <= verdicts, verdicts


def test_parity_on_every_foreign_frame(ZT, torch, tmp_path, golden_dir):
    """every case of foreign_frames.json as an entry of one archive, in one batch"""
    cases = _load(golden_dir, "foreign_frames.json")
    frames = [bytes.fromhex(c["frame"]) for c in cases]
    ents, pos = [], 10
    for k, (c, fr) in enumerate(zip(cases, frames)):
        ents.append(("f%02d" % k, pos, len(fr), c["uncomp_size"], c["hash"], c["method"]))
        pos += len(fr)
    arc = zpk.assemble(frames + [b"\0" * 16], ents)
    rc, res, last = _parity(ZT, torch, tmp_path, arc)
    assert len(res) == 61
    for c, v in zip(cases, res):
        if c["max_size"] == c["uncomp_size"]:
            assert v == c["rc"], (c["label"], v, c["rc"])                              # the reference's recorded verdict, where its buffer was an exact one


def test_parity_on_the_synthetic_archive_and_its_routes(ZT, torch, tmp_path, codec, synth):
    arc, specs = synth["arc"], synth["specs"]
    assert _parity(ZT, torch, tmp_path, arc) == (0, [0] * len(specs), 0)
    res, st_host, st_dimage = _codec_parity(codec, torch, arc, _desc_of(arc))
    assert [int(x) for x in res["produced"]] == [len(s[2]) for s in specs]
    assert all(int(h) == oracle().xxh3(s[2]) for s, h in zip(specs, res["hash"]) if s[2])
    print("routes: host %s, device image %s" % ({k: st_host[k] for k in ROUTES}, {k: st_dimage[k] for k in ROUTES}))
    assert st_host["frame_parallel_entries"] >= 2                                      # the 320 KiB and 1.5 MiB compressed entries: block-parallel at the default ZPK_OPT_DEC_SPLIT_MIN
    assert st_dimage["frame_parallel_entries"] >= 2 and st_dimage["device_walk_accepted"] >= 2
    assert st_dimage["stored_span_entries"] == 2                                       # the 320 KiB and the 1.5 MiB stored entry: chip-wide
    # the empty entry in the middle, alone and between two others
    mid = _index(0, dg.LZ4)
    assert _parity(ZT, torch, tmp_path, arc, picks=[mid]) == (0, [0], 0)
    assert _parity(ZT, torch, tmp_path, arc, picks=[mid - 3, mid, mid + 3]) == (0, [0, 0, 0], 0)
    # the 320 KiB stored entry on its own: the chip-wide stored route of a device image
    one = _index(320 << 10, dg.NONE)
    assert _parity(ZT, torch, tmp_path, arc, picks=[one]) == (0, [0], 0)
    image = _image(torch, arc, 1)[1:1 + len(arc)]
    r = codec.verify_batch_dimage(image, _desc_of(arc)[one:one + 1])
    assert int(r[0]["status"]) == 0 and int(r[0]["hash"]) == oracle().xxh3(specs[one][2]) and codec.decode_stats()["stored_span_entries"] == 1
    assert codec.verify_stats() == dict(sub_batches=1, stored_hashed_in_place=1, bytes_copied_home=0)


# ------------------------------------------------------------------------------------------------ 2. damage

def test_damage_gets_the_read_paths_verdicts(ZT, torch, tmp_path, codec, synth):
    arc = bytearray(synth["arc"])
    pe = zpk.parse(arc)
    flipped = [_index(65536, m) for m in (dg.NONE, dg.LZ4, dg.ZSTD)] + [_index(3 << 19, dg.LZ4), _index(320 << 10, dg.ZSTD), _index(320 << 10, dg.NONE)]
    for i in flipped:                                                                  # one payload byte per entry kind, the large routes included
        arc[pe[i]["offset"] + pe[i]["comp_size"] // 2] ^= 0x10
    magic = _index(1024, dg.ZSTD)
    arc[pe[magic]["offset"]] ^= 0xFF                                                   # a destroyed frame magic
    arc = bytes(arc)
    wrong_hash, short_comp = _index(1025, dg.LZ4), _index(241, dg.NONE)
    ptam = {wrong_hash: {"hash": pe[wrong_hash]["hash"] ^ 1}, short_comp: {"comp_size": pe[short_comp]["comp_size"] - 1}}
    rc, res, last = _parity(ZT, torch, tmp_path, arc, tamper=ptam)
    assert rc == 0 and res[wrong_hash] == 15 and res[short_comp] == 18 and res[magic] != 0
    assert all(res[i] != 0 for i in flipped) and res[flipped[0]] == 15 and res[flipped[5]] == 15
    assert [i for i, v in enumerate(res) if v != 0] == sorted(flipped + [magic, wrong_hash, short_comp])     # one bad entry does not stop the others
    vres, st_host, st_dimage = _codec_parity(codec, torch, arc, _desc_of(arc, ptam))
    assert [int(x) for x in vres["status"]] == res
    stored_ok = sum(1 for k, s in enumerate(synth["specs"]) if s[0] == dg.NONE and len(s[2]) and k != short_comp)
    assert codec.verify_stats()["stored_hashed_in_place"] == stored_ok == 7            # (the last call: the device image)


# ------------------------------------------------------------------------------------------------ 3. short decodes

@pytest.mark.parametrize("n", [5000, 300000])
def test_a_short_decode_is_hashed_with_zeros_behind_it(ZT, torch, tmp_path, codec, n):
    """an LZ4 frame and a Zstandard frame of n bytes entered with uncomp_size = n + 37 and the XXH3 of the plaintext followed by 37 zero bytes"""
    plain = [_plain(0, n), _plain(3, n)]
    frames = [dg.compress(dg.LZ4, 0, plain[0]), dg.compress(dg.ZSTD, 3, plain[1])]
    noise = _plain(1, 2 * n + 4096)                                                    # random bytes: an LZ4 frame of stored blocks, decoded over both slots
    other = dg.compress(dg.LZ4, 0, noise)
    hashes = [oracle().xxh3(p + bytes(37)) for p in plain]
    ents, pos = [], 10
    for name, fr, size, h, m in (("lz4", frames[0], n + 37, hashes[0], dg.LZ4), ("zstd", frames[1], n + 37, hashes[1], dg.ZSTD), ("noise", other, len(noise), dg.xxh3(noise), dg.LZ4)):
        ents.append((name, pos, len(fr), size, h, m))
        pos += len(fr)
    arc = zpk.assemble(frames + [other, b"\0" * 16], ents)
    for kind in KINDS:
        r, keep = _open(ZT, torch, kind, arc, tmp_path)
        try:
            short, between = _entries(r, [0, 1]), _entries(r, [2])
            assert _read(ZT, r, short, 0x00) == (0, [0, 0], 0), kind
            assert _read(ZT, r, short, 0xFF)[:2] == (0, [15, 15]), kind                # the fixture bites: the reference hashes what the buffer held
            assert _test(ZT, r, short) == (0, [0, 0], 0), kind
            assert _test(ZT, r, between) == (0, [0], 0), kind                          # another batch over the same staging ...
            assert _test(ZT, r, short) == (0, [0, 0], 0), kind                         # ... and stale bytes behind the decoded ones do not show
        finally:
            ZT.lib.zpack_close_reader(C.byref(r))
    desc = _desc_of(arc)
    res = codec.verify_batch_host(arc, desc[:2])
    assert [(int(x["status"]), int(x["produced"]), int(x["hash"])) for x in res] == [(0, n, hashes[0]), (0, n, hashes[1])]
    codec.verify_batch_host(arc, desc[2:])
    image = _image(torch, arc, 9)[9:9 + len(arc)]
    for _ in range(2):
        res = codec.verify_batch_dimage(image, desc)
        assert [(int(x["status"]), int(x["produced"]), int(x["hash"])) for x in res[:2]] == [(0, n, hashes[0]), (0, n, hashes[1])] and int(res[2]["status"]) == 0
    desc["expect_hash"][0] ^= 1
    assert [int(x) for x in codec.verify_batch_host(arc, desc)["status"]] == [15, 0, 0]


# ------------------------------------------------------------------------------------------------ 4. nothing comes home, nothing is copied

def test_nothing_comes_home_and_nothing_is_copied(codec, torch, synth):
    arc, specs = synth["arc"], synth["specs"]
    desc = _desc_of(arc)
    stored = sum(1 for s in specs if s[0] == dg.NONE and len(s[2]))
    image = _image(torch, arc, 2)[2:2 + len(arc)]
    outs = [torch.empty(max(1, len(s[2])), dtype=torch.uint8, device="cuda:0") for s in specs]
    codec.decode_batch_dimage(image, desc, [t.data_ptr() for t in outs])               # (a call that does launch k_span_copy)
    assert codec.dimage_stats()["span_copy_launches"] == 1
    res = codec.verify_batch_host(arc, desc)
    assert (res["status"] == 0).all() and codec.verify_stats() == dict(sub_batches=1, stored_hashed_in_place=stored, bytes_copied_home=0)
    assert codec.decode_stats()["span_copy_launches"] == 0
    res = codec.verify_batch_dimage(image, desc)
    assert (res["status"] == 0).all() and codec.verify_stats() == dict(sub_batches=1, stored_hashed_in_place=stored, bytes_copied_home=0)
    assert codec.dimage_stats() == dict(sub_batches=1, span_copy_launches=0, bytes_copied_home=0)
    codec.decode_batch_host(arc, desc)                                                 # the read it replaces does bring the plaintext home
    assert codec.verify_stats()["bytes_copied_home"] >= sum(len(s[2]) for s in specs)


# ------------------------------------------------------------------------------------------------ 5. the hash-only kernel against the oracle's XXH3

def test_stored_entries_hashed_in_place_at_every_length_and_alignment(codec, torch):
    lens = list(range(1, 301)) + [1023, 1024, 1025, 2047, 2048, 2049, 65535, 65536, 65537]
    rng = np.random.default_rng(23)
    o = oracle()
    want = {}
    pos, rows = 256, []
    for n in lens:
        data = rng.integers(0, 256, n, dtype=np.uint8)
        want[n] = o.xxh3(data)
        for a in range(16):
            pos = ((pos + 15) & ~15) + a                                               # the payload begins at an address = a mod 16 (the image itself is 256-aligned)
            rows.append((pos, n, data))
            pos += n + 1
    blob = rng.integers(0, 256, pos + 64, dtype=np.uint8)
    desc = np.zeros(len(rows), dtype=zpack_amd.DECODE_DESC)
    for d, (at, n, data) in zip(desc, rows):
        blob[at:at + n] = data
        d["src_offset"], d["comp_size"], d["uncomp_size"], d["expect_hash"], d["method"] = at, n, n, want[n], dg.NONE
    image = torch.from_numpy(blob).to("cuda:0")
    torch.cuda.synchronize()
    assert image.data_ptr() % 256 == 0
    hashes = np.array([want[n] for _, n, _ in rows], dtype=np.uint64)
    for call, src in ((codec.verify_batch_dimage, image), (codec.verify_batch_host, blob)):
        res = call(src, desc)
        bad = np.flatnonzero((res["status"] != 0) | (res["hash"] != hashes) | (res["produced"] != desc["uncomp_size"]) | (res["detail"] != 0))
        assert len(bad) == 0, [(rows[i][0] % 16, rows[i][1], res[i]) for i in bad[:5]]
        assert codec.verify_stats() == dict(sub_batches=1, stored_hashed_in_place=len(rows), bytes_copied_home=0)
        assert codec.decode_stats()["stored"] == len(rows)                             # one wave each: none is large enough for the chip-wide route
        wrong = desc.copy()
        wrong["expect_hash"] ^= np.uint64(1 << 40)
        res = call(src, wrong)
        assert (res["status"] == 15).all() and (res["hash"] == hashes).all()
        wrong["flags"] = zpack_amd.DF_SKIP_HASH
        res = call(src, wrong)
        assert (res["status"] == 0).all() and (res["hash"] == hashes).all()


# ------------------------------------------------------------------------------------------------ 6. sub-batches

def test_sub_batches_by_the_chunk_option_on_both_calls(codec, torch, synth):
    arc = synth["arc"]
    desc = _desc_of(arc)
    image = _image(torch, arc, 4)[4:4 + len(arc)]
    one = {}
    for name, call, src in (("host", codec.verify_batch_host, arc), ("dimage", codec.verify_batch_dimage, image)):
        one[name] = call(src, desc)
        assert codec.verify_stats()["sub_batches"] == 1 and (one[name]["status"] == 0).all()
    codec.set_option(zpack_amd.OPT_DIMAGE_CHUNK, 1 << 20)
    try:
        for name, call, src in (("host", codec.verify_batch_host, arc), ("dimage", codec.verify_batch_dimage, image)):
            res = call(src, desc)
            s = codec.verify_stats()
            print("%s: %s" % (name, s))
            assert s["sub_batches"] >= 1 and s["bytes_copied_home"] == 0 and (name == "host" or s["sub_batches"] > 1)
            assert res.tobytes() == one[name].tobytes()
        # The host form takes its large entries out of the batch first (groups of frames, block-parallel turns), and what is left of this
        # archive is less than one chunk: with those routes off, the chunk cuts the whole batch there too
        codec.set_option(zpack_amd.OPT_DEC_SPLIT_MIN, 0)
        res = codec.verify_batch_host(arc, desc)
        s = codec.verify_stats()
        print("host, one wave per entry: %s" % s)
        assert s["sub_batches"] > 1 and s["bytes_copied_home"] == 0 and res.tobytes() == one["host"].tobytes()
    finally:
        codec.set_option(zpack_amd.OPT_DIMAGE_CHUNK, 0)
        codec.set_option(zpack_amd.OPT_DEC_SPLIT_MIN, 256 << 10)


def _cut_model(slots, chunk):
    """the sub-batches of staging slots at `chunk`: a sub-batch closes when the next slot would take it past the chunk, its first
    entry always joins (host_plan.h / dimage_plan.h state this; the count here comes from this loop alone)"""
    subs, total, count = [], 0, 0
    for s in slots:
        if count and (total > chunk or s > chunk - total):
            subs.append((count, total))
            total = count = 0
        total, count = total + s, count + 1
    return subs + ([(count, total)] if count else [])


def test_both_calls_cut_the_same_sub_batches_and_an_entry_above_the_chunk_goes_alone(codec, torch):
    """12 entries of 4 KiB to 96 KiB, stored, LZ4 and Zstandard in turn, at a chunk of 64 KiB: the slot of the 96 KiB LZ4 entry exceeds it"""
    sizes = [4 << 10, 96 << 10, 8 << 10, 20000, 40 << 10, 4097, 64 << 10, 12 << 10, 33333, 16 << 10, 50 << 10, 24 << 10]
    specs = [METHODS[i % 3] + (_plain(i, n),) for i, n in enumerate(sizes)]
    arc = _build(specs)
    desc = _desc_of(arc)
    image = _image(torch, arc, 6)[6:6 + len(arc)]
    chunk = 64 << 10
    slots = [0 if m == dg.NONE else (n + 255) & ~255 for (m, _, _), n in zip(specs, sizes)]      # (no destination: a stored entry has no slot)
    want = _cut_model(slots, chunk)
    assert (1, (96 << 10)) in want and len(want) > 2, want
    read, _ = codec.decode_batch_host(arc, desc)
    assert (read["status"] == 0).all() and [int(h) for h in read["hash"]] == [oracle().xxh3(s[2]) for s in specs]
    codec.set_option(zpack_amd.OPT_DIMAGE_CHUNK, chunk)
    try:
        subs = {}
        for name, call, src in (("host", codec.verify_batch_host, arc), ("dimage", codec.verify_batch_dimage, image)):
            res = call(src, desc)
            subs[name] = codec.verify_stats()["sub_batches"]
            assert res.tobytes() == read.tobytes(), name
        print("sub-batches: %s, the model: %s" % (subs, want))
        assert subs["host"] == subs["dimage"] == len(want)
    finally:
        codec.set_option(zpack_amd.OPT_DIMAGE_CHUNK, 0)


# ------------------------------------------------------------------------------------------------ 7. the pipelined upload is kept

def test_a_large_host_batch_keeps_its_pipelined_upload(codec):
    """12 288 x 16 KiB LZ4 entries: 128 generated, their payloads repeated 96 times in the image"""
    b = dg.Batch(128, 16384, method=dg.LZ4, level=0, seed=11)
    lo, hi = int(b.offsets[0]), int(b.offsets[-1] + b.comp_sizes[-1])
    region = b.archive[lo:hi]
    reps, n = 96, 96 * 128
    image = np.concatenate([np.zeros(10, dtype=np.uint8), np.tile(region, reps), np.zeros(64, dtype=np.uint8)])
    desc = np.zeros(n, dtype=zpack_amd.DECODE_DESC)
    rel = (b.offsets - np.uint64(lo)).astype(np.uint64)
    desc["src_offset"] = (np.uint64(10) + np.repeat(np.arange(reps, dtype=np.uint64) * np.uint64(hi - lo), 128) + np.tile(rel, reps))
    desc["comp_size"], desc["uncomp_size"] = np.tile(b.comp_sizes, reps), np.tile(b.uncomp_sizes, reps)
    desc["expect_hash"], desc["method"] = np.tile(b.hashes, reps), dg.LZ4
    res = codec.verify_batch_host(image, desc)
    st = codec.decode_stats()
    assert st["pipelined_sub_batches"] >= 1, st                                        # ZPK_DS2_PIPE_SUBS
    assert (res["status"] == 0).all() and (res["hash"] == desc["expect_hash"]).all() and st["lz4"] == n
    assert codec.verify_stats() == dict(sub_batches=1, stored_hashed_in_place=0, bytes_copied_home=0)
    bad = 7777
    desc["expect_hash"][bad] ^= np.uint64(1)
    res = codec.verify_batch_host(image, desc)
    assert codec.decode_stats()["pipelined_sub_batches"] >= 1
    assert [int(i) for i in np.flatnonzero(res["status"] != 0)] == [bad] and int(res[bad]["status"]) == 15
    b.close()


# ------------------------------------------------------------------------------------------------ 8. the torch view

def test_device_io_test_files(torch, tmp_path, synth):
    from zpack_amd import device_io
    arc, specs = synth["arc"], synth["specs"]
    path = os.path.join(str(tmp_path), "synth.zpk")
    with open(path, "wb") as fh:
        fh.write(arc)
    assert device_io.test_files(path) == [0] * len(specs)
    assert device_io.test_files(arc) == [0] * len(specs)
    assert device_io.test_files(arc, names=["e0020", "e0003"]) == [0, 0]
    tensors = {"t%d" % i: torch.from_numpy(np.frombuffer(_plain(3 * i, 50000 + 4097 * i), dtype=np.uint8).copy()).to("cuda:0") for i in range(5)}
    image = device_io.write_archive_device(tensors, method=device_io.METHOD_LZ4, level=0)
    before = torch.cuda.memory_allocated(0)
    assert device_io.test_files(image) == [0] * 5
    assert torch.cuda.memory_allocated(0) == before                                    # no tensor was allocated
    e = zpk.parse(image.cpu().numpy().tobytes())[2]
    image[e["offset"] + e["comp_size"] // 2] ^= 0x04                                   # one byte of the image flipped on the device
    torch.cuda.synchronize()
    st = device_io.test_files(image)
    assert st[2] != 0 and [v for k, v in enumerate(st) if k != 2] == [0] * 4
    with pytest.raises(ValueError):
        device_io.test_files(image.to(torch.int8))


# ------------------------------------------------------------------------------------------------ 9. read-ahead untouched; contexts

def test_read_ahead_is_neither_used_nor_fed(ZT, torch, tmp_path):
    specs = [((dg.LZ4, 0), (dg.ZSTD, 3), (dg.NONE, 0))[i % 3] + (_plain(i, 1500 + 37 * i),) for i in range(40)]
    arc = _build(specs)
    for kind in ("memory", "device"):
        r, keep = _open(ZT, torch, kind, arc, tmp_path)
        try:
            def read(i):
                n = len(specs[i][2])
                out = np.zeros(n + 1, dtype=np.uint8)
                assert ZT.lib.zpack_read_file(C.byref(r), C.pointer(r.file_entries[i]), out.ctypes.data, n, None) == 0
                assert out[:n].tobytes() == specs[i][2]

            def stats():
                s = (C.c_uint64 * 6)()
                assert ZT.lib.zpack_amd_read_ahead_stats(C.byref(r), None, s) == 0
                return list(s)

            for i in range(20):                                                        # the middle of an in-order run
                read(i)
            before = stats()
            assert before[0] > 0 and before[2] > 0, before
            assert _test(ZT, r, _entries(r)) == (0, [0] * 40, 0)
            assert stats() == before
            for i in range(20, 40):
                read(i)
            after = stats()
            assert after[0] > before[0], (before, after)                               # the run went on out of its windows
        finally:
            ZT.lib.zpack_close_reader(C.byref(r))


def test_a_context_over_several_codecs_shards_the_test_call(ZT, torch, tmp_path, synth):
    """ZPACK_AMD_DEVICES rehearsed on one card as "0,0,0": a memory and a file reader shard as zpack_read_files does"""
    arc = bytearray(synth["arc"])
    pe = zpk.parse(arc)
    bad = _index(65536, dg.ZSTD)
    arc[pe[bad]["offset"] + 100] ^= 0x20
    old = os.environ.get("ZPACK_AMD_DEVICES")
    os.environ["ZPACK_AMD_DEVICES"] = "0,0,0"
    try:
        rc, res, last = _parity(ZT, torch, tmp_path, bytes(arc), kinds=("memory", "file"))
        assert rc == 0 and [i for i, v in enumerate(res) if v != 0] == [bad]
    finally:
        if old is None:
            del os.environ["ZPACK_AMD_DEVICES"]
        else:
            os.environ["ZPACK_AMD_DEVICES"] = old


def test_an_image_on_a_device_the_context_does_not_hold(ZT, torch, golden_dir):
    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    arc = open(os.path.join(golden_dir, "ref_workdir", "archive_lz4.zpk"), "rb").read()
    t = torch.from_numpy(np.frombuffer(arc, dtype=np.uint8).copy()).to("cuda:1")
    torch.cuda.synchronize(1)
    r = Reader()
    assert ZT.lib.zpack_amd_init_reader_device(C.byref(r), t.data_ptr(), len(arc)) == 0
    try:
        rc, res, last = _test(ZT, r, _entries(r))
        assert (rc, res) in ((NOT_AVAILABLE, [-1, -1]), (0, [0, 0]))                   # NOT_AVAILABLE: the reader's context (ZPACK_AMD_DEVICES) has no codec on the image's device
    finally:
        ZT.lib.zpack_close_reader(C.byref(r))
