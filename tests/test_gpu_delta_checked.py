"""GPU: the base of a delta entry is hashed on the device before it is applied (include/zpack_amd.h: zpack_amd_hash_device,
zpack_amd_read_files_device_delta_checked; the codec's _delta_checked calls behind them).

Six entries written by the existing delta call — element sizes 2, 2, 4, 8, 1, 2; 1 KiB + 3, 16 KiB, 48 KiB + 2, 300 KiB (a candidate
of the block-parallel readers, which stage it because of its base), 5 bytes, and one entry without a base — into a heap writer and a device sink, LZ4 and Zstandard level 1, read through a
memory reader and a device image.  The reference of a read with the right bases is the existing _delta read: its results and bytes,
byte for byte.  The values the bases have to hash to come from the CPU XXH3 of the oracle, not from the code under test."""
import ctypes as C

import numpy as np
import pytest

from tests._libs import Reader, FileEntry, oracle, METHOD_ZSTD, METHOD_LZ4
from tests.device_mem import torch, Z, _layout, CANARY            # noqa: F401  (torch, Z: fixtures)
from tests.test_gpu_planes_io import _on_device, Opened, _want, _same, MIS, PFE
from tests.test_gpu_delta_io import D, _write                     # noqa: F401  (D: a fixture)

pytestmark = pytest.mark.gpu

OK, HASH_MISMATCH, BASE_MISMATCH = 0, 15, 64
METHODS = [pytest.param((METHOD_LZ4, 0), id="lz4"), pytest.param((METHOD_ZSTD, 1), id="zstd1")]
NAMES = ["a.1k3", "b.16k", "c.48k2", "d.300k", "e.5", "f.nobase"]
ELEM = [2, 2, 4, 8, 1, 2]
SIZES = [1024 + 3, 16 << 10, (48 << 10) + 2, 300 << 10, 5, 2049]
BASED = [0, 1, 2, 3, 4]                                                                # entry 5 has no base


@pytest.fixture(scope="module")
def K(D):
    L = D.lib
    R, vp, u64 = C.POINTER(Reader), C.c_void_p, C.c_uint64
    L.zpack_amd_read_files_device_delta_checked.argtypes = [R, C.POINTER(PFE), u64, vp, C.POINTER(C.c_size_t), C.POINTER(C.c_uint8), C.POINTER(vp), C.POINTER(u64),
                                                            C.POINTER(C.c_int), vp]
    L.zpack_amd_hash_device.argtypes = [C.POINTER(vp), C.POINTER(C.c_size_t), u64, C.POINTER(u64), vp]
    return D


@pytest.fixture(scope="module")
def data():
    """the tensors' bytes, their bases — the tensor with one byte of twenty replaced — and the CPU XXH3 of every base; computed once"""
    rng = np.random.default_rng(30)
    arrays = [rng.integers(0, 256, n, dtype=np.uint8) for n in SIZES]
    bases = []
    for i, a in enumerate(arrays):
        b = a.copy()
        hit = rng.random(a.size) < 0.05
        b[hit] = rng.integers(0, 256, int(hit.sum()), dtype=np.uint8)
        bases.append(b if i in BASED else None)
    o = oracle()
    hashes = [o.xxh3(b.tobytes()) if b is not None else 0x0BADBADBADBADBAD for b in bases]      # (the entry without a base: a value nobody looks at)
    return dict(arrays=arrays, bases=bases, hashes=hashes)


@pytest.fixture(scope="module", params=METHODS)
def made(request, K, torch, data):
    """one method: the image the existing delta call writes into a heap writer; the device sink writes the same bytes"""
    mc = request.param
    rc, image, ents, _ = _write(K, torch, NAMES, data["arrays"], mc, ELEM, data["bases"], "heap")
    assert rc == OK and len(ents) == len(NAMES)
    rc, dimage, dents, _ = _write(K, torch, NAMES, data["arrays"], mc, ELEM, data["bases"], "device")
    assert rc == OK and dimage == image and dents == ents
    return dict(data, mc=mc, image=image, ents=ents)


def _flipped(b):
    """the base with a single bit flipped in its last byte"""
    x = b.copy()
    x[-1] ^= 0x10
    return x


def _read(K, torch, o, ents, bases, hashes, call, inplace=False, idx=None):
    """Entries idx (all) read into canaried device buffers, or in place into buffers that hold `bases` and ARE the bases.
    -> (rc, results), the destination buffer afterwards, the destinations' offsets, the bases' buffer before and afterwards (elsewhere)"""
    idx = list(range(len(NAMES))) if idx is None else idx
    n = len(idx)
    caps = [SIZES[i] for i in idx]
    offs, total = _layout(caps, MIS)
    h = np.full(total, CANARY, dtype=np.uint8)
    if inplace:
        for x, b in zip(offs, bases):
            if b is not None:
                h[x:x + b.size] = b
    buf = torch.from_numpy(h).to("cuda:0")
    bbuf, baddr, bbefore = _on_device(torch, [b if b is not None else np.zeros(0, dtype=np.uint8) for b in bases], mis=(1, 15, 0, 3))
    torch.cuda.synchronize()
    dst = [buf.data_ptr() + x for x in offs]
    c_bases = (C.c_void_p * n)(*[None if b is None else (d if inplace else x) for b, x, d in zip(bases, baddr, dst)])
    ptrs = (PFE * n)(*[C.pointer(e) for e in ents])
    res = (C.c_int * n)(*([-1] * n))
    csz = (C.c_size_t * n)(*caps)
    c_elem = (C.c_uint8 * n)(*[ELEM[i] for i in idx])
    if call == "delta":
        rc = K.lib.zpack_amd_read_files_device_delta(C.byref(o.r), ptrs, n, (C.c_void_p * n)(*dst), csz, c_elem, c_bases, res, None)
    else:
        c_hash = None if hashes is None else (C.c_uint64 * n)(*hashes)
        rc = K.lib.zpack_amd_read_files_device_delta_checked(C.byref(o.r), ptrs, n, (C.c_void_p * n)(*dst), csz, c_elem, c_bases, c_hash, res, None)
    torch.cuda.synchronize()
    assert np.array_equal(bbuf.cpu().numpy(), bbefore)                                  # bases that are not destinations are only read
    return (rc, list(res)), buf.cpu().numpy(), offs


def test_hash_device_gives_the_cpu_xxh3_of_the_bases_and_of_nothing(K, torch, data):
    bases = [b if b is not None else np.zeros(0, dtype=np.uint8) for b in data["bases"]]
    buf, addr, before = _on_device(torch, bases, mis=(3, 1, 15, 0))
    n = len(bases)
    out = (C.c_uint64 * n)()
    rc = K.lib.zpack_amd_hash_device((C.c_void_p * n)(*addr), (C.c_size_t * n)(*[b.size for b in bases]), n, out, None)
    assert rc == OK
    assert list(out)[:5] == data["hashes"][:5] and out[5] == oracle().xxh3(b"")
    assert np.array_equal(buf.cpu().numpy(), before)
    host = np.zeros(64, dtype=np.uint8)                                                 # host memory is no device span: refused, nothing written
    out1 = (C.c_uint64 * 1)(7)
    assert K.lib.zpack_amd_hash_device((C.c_void_p * 1)(host.ctypes.data), (C.c_size_t * 1)(64), 1, out1, None) == 21 and out1[0] == 7


@pytest.mark.parametrize("split", ["default-split", "split-64k"])
@pytest.mark.parametrize("where", ["memory", "device"])
def test_right_bases_are_the_delta_read_byte_for_byte_and_null_hashes_are_the_delta_call(K, torch, made, where, split, monkeypatch):
    """(a), (e), (f).  split-64k: the reader's own context, created by its first read, offers entries from 64 KiB to the block-parallel
    readers (the default is 256 KiB, which the 300 KiB entry passes either way)"""
    if split == "split-64k":
        monkeypatch.setenv("ZPACK_AMD_DEC_SPLIT_MIN", "65536")
    m = made
    o = Opened(K, torch, m["image"], where)
    try:
        for inplace in (False, True):
            headd, bufd, offs = _read(K, torch, o, o.ents, m["bases"], None, "delta", inplace)
            assert headd == (OK, [OK] * 6)
            _same(bufd, _want(bufd.size, offs, m["arrays"]), "the delta read gives the tensors")
            head, buf, _ = _read(K, torch, o, o.ents, m["bases"], m["hashes"], "checked", inplace)
            assert head == headd
            _same(buf, bufd, ("(a) right bases", inplace))
            head, buf, _ = _read(K, torch, o, o.ents, m["bases"], None, "checked", inplace)
            assert head == headd
            _same(buf, bufd, ("(e) no hashes", inplace))
            other = list(m["hashes"]); other[5] ^= 0xFFFF                               # (f) the entry without a base: whatever value
            head, buf, _ = _read(K, torch, o, o.ents, m["bases"], other, "checked", inplace)
            assert head == headd
            _same(buf, bufd, ("(f) the value of an entry without a base", inplace))
    finally:
        o.close()


@pytest.mark.parametrize("where", ["memory", "device"])
def test_a_base_with_one_bit_flipped_is_refused_and_nothing_of_it_is_written(K, torch, made, where):
    """(b), (c): every entry with a base in turn, its base wrong in one bit of its last byte.
    THE PARENT: the same read through zpack_amd_read_files_device_delta answers ZPACK_OK for that entry and writes tensor XOR (one bit) —
    garbage the caller cannot tell from the tensor —, in place over the only copy of the previous checkpoint; asserted below, because that
    call is unchanged.  The checked call: BASE_MISMATCH, the destination untouched, every other entry delivered."""
    m = made
    o = Opened(K, torch, m["image"], where)
    try:
        for j in BASED:
            bases = list(m["bases"]); bases[j] = _flipped(bases[j])
            for inplace in (False, True):
                head, buf, offs = _read(K, torch, o, o.ents, bases, None, "delta", inplace)
                assert head == (OK, [OK] * 6)                                           # (the parent's answer: nothing noticed)
                wrong = m["arrays"][j].copy(); wrong[-1] ^= 0x10
                assert np.array_equal(buf[offs[j]:offs[j] + SIZES[j]], wrong)           # (... and garbage delivered)
                head, buf, offs = _read(K, torch, o, o.ents, bases, m["hashes"], "checked", inplace)
                assert head == (OK, [BASE_MISMATCH if i == j else OK for i in range(6)]), (j, inplace)
                # (b) canaries where the tensor would have gone; (c) in place: the base buffer, bit for bit what it was
                kept = bases[j] if inplace else None
                _same(buf, _want(buf.size, offs, [kept if i == j else a for i, a in enumerate(m["arrays"])]), (j, inplace))
        # every base wrong at once: nothing with a base is delivered, the entry without one is
        bases = [_flipped(b) if b is not None else None for b in m["bases"]]
        head, buf, offs = _read(K, torch, o, o.ents, bases, m["hashes"], "checked", True)
        assert head == (OK, [BASE_MISMATCH] * 5 + [OK])
        _same(buf, _want(buf.size, offs, bases[:5] + [m["arrays"][5]]), "all refused, in place")
    finally:
        o.close()


def _payload_flip_that_only_breaks_the_hash(image, ent, method):
    """a byte of the entry's payload whose flip still decodes to all of its bytes, other ones: FILE_HASH_MISMATCH by the CPU oracle"""
    off, comp, unc, h, _ = ent
    o = oracle()
    for at in list(range(off + comp - 5, off + comp // 2, -1)):
        broken = bytearray(image); broken[at] ^= 0x01
        rc, _, got, _ = o.entry_decode(bytes(broken), off, comp, unc, h, method, unc)
        if rc == HASH_MISMATCH and got == unc:
            return bytes(broken)
    pytest.fail("no payload byte whose flip gives FILE_HASH_MISMATCH")


@pytest.mark.parametrize("where", ["memory", "device"])
def test_a_damaged_entry_with_a_wrong_base(K, torch, made, where):
    """(d): a flipped stored byte decodes and fails its hash — delivered by the _delta call, so BASE_MISMATCH replaces it; a truncated
    frame is not delivered by either call and keeps its own status.  The neighbours are delivered."""
    m = made
    j = 1                                                                               # the 16 KiB entry
    idx = [0, 1, 2]
    bases = [m["bases"][i] for i in idx]
    wrong = list(bases); wrong[1] = _flipped(bases[1])
    hashes = [m["hashes"][i] for i in idx]
    image = _payload_flip_that_only_breaks_the_hash(m["image"], m["ents"][j], m["mc"][0])
    o = Opened(K, torch, image, where)
    try:
        ents = [o.ents[i] for i in idx]
        head, _, _ = _read(K, torch, o, ents, bases, hashes, "checked", idx=idx)
        assert head == (OK, [OK, HASH_MISMATCH, OK])                                    # the right base: the entry's own status, delivered as ever
        for inplace in (False, True):
            head, buf, offs = _read(K, torch, o, ents, wrong, hashes, "checked", inplace, idx=idx)
            assert head == (OK, [OK, BASE_MISMATCH, OK]), inplace
            _same(buf, _want(buf.size, offs, [m["arrays"][0], wrong[1] if inplace else None, m["arrays"][2]]), ("flipped byte", inplace))
        cut = FileEntry.from_buffer_copy(o.ents[j])
        cut.comp_size -= 9                                                              # the frame's last bytes are not the entry's
        ents = [o.ents[0], cut, o.ents[2]]
        headd, _, _ = _read(K, torch, o, ents, wrong, None, "delta", idx=idx)
        assert headd[0] == OK and headd[1][1] not in (OK, HASH_MISMATCH, BASE_MISMATCH)
        for inplace in (False, True):
            head, buf, offs = _read(K, torch, o, ents, wrong, hashes, "checked", inplace, idx=idx)
            assert head == headd, inplace                                               # its own status, not the base's
            _same(buf, _want(buf.size, offs, [m["arrays"][0], wrong[1] if inplace else None, m["arrays"][2]]), ("truncated", inplace))
    finally:
        o.close()
