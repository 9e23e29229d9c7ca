"""zpk_codec_pack_batch_device alone, against numpy (tests/pack_cases.py; tests/test_pack_cases_cpu.py judges that file on the CPU).

Every other test reaches the size scan and the gather through a real encode, with the sizes the encoder happened to give.  Here `desc`
and `results` are written by the test and uploaded, so the call sees what no encoder produces on demand: more than 262 144 entries (the
second trip of k_pack_scan_blocks' loop), sums past 2^32 (the high half of every shuffle), failed entries with a garbage comp_size in
runs that fill a wave and a block, payloads of every length around 16, 64 and PK_SPAN at every residue of the slot and of the packed
address, a packed base off a 16-byte boundary, a packed buffer that is too short, and the two refusals of the launch sizing.

Every packed buffer is a slice of a larger allocation: GUARD_FRONT bytes in front of the base, and behind it the whole packed stream
plus GUARD_BEHIND bytes whatever packed_cap says.  Everything runs under two fills.  P.check states what is asserted of a call.

NOT asserted: which of the bytes in front of packed_cap of an entry that crosses it are written (the contract leaves it open), what
`offsets` holds after the second refusal, and timing."""
import ctypes as C

import numpy as np
import pytest

import zpack_amd
from benchdata import datagen as dg
from tests import pack_cases as P
from tests.test_enc_capacity_cpu import min_capacity

pytestmark = pytest.mark.gpu

E_INVALID = r"zpk_codec_pack_batch_device failed \(-2\)"            # ZPK_E_INVALID (include/zpack_codec.h)


@pytest.fixture(scope="module")
def codec():
    c = zpack_amd.Codec(0)
    yield c
    c.close()


class Span:
    """what Codec.pack_batch_device asks of `packed`: an address and a length.  A torch slice cannot say "zero bytes AT this address"
    (an empty tensor's data_ptr is NULL, which the call takes as "sizes only"), and packed_cap is the length of the slice."""

    def __init__(self, ptr, n):
        self.ptr, self.n = ptr, n

    def data_ptr(self):
        return self.ptr

    def numel(self):
        return self.n


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(torch.device("cuda:0"))


def _filled(nbytes, fill):
    import torch
    return torch.full((nbytes,), fill, dtype=torch.uint8, device=torch.device("cuda:0"))


class OnDevice:
    """a gather case uploaded once: slots, desc and results as the call takes them"""

    def __init__(self, g):
        self.g, self.n = g, len(g.res)
        self.slots, self.desc, self.res = _up(g.slots), _up(g.desc), _up(g.res)

    def slots_unchanged(self):
        return np.array_equal(self.slots.cpu().numpy(), self.g.slots)


@pytest.fixture(scope="module")
def on_device():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = OnDevice(P.gather_cases()[name])
        return cache[name]
    return get


def _pack(codec, d, total, fill, off=0, cap=None, max_entry_size=None, stream=None):
    """One call with a packed buffer -> (offsets as the device left them, the whole allocation, lead).  The packed base is byte `lead`
    of the allocation, `off` bytes behind a 16-byte boundary; the allocation holds `total` bytes and GUARD_BEHIND more behind the base
    whatever `cap` (packed_cap; default: exactly total) is."""
    import torch
    whole = _filled(P.GUARD_FRONT + 16 + total + P.GUARD_BEHIND, fill)
    lead = P.GUARD_FRONT + (off - whole.data_ptr()) % 16
    offs = _filled(8 * (d.n + 1), fill)
    packed = Span(whole.data_ptr() + lead, total if cap is None else cap)
    assert packed.data_ptr() % 16 == off and lead + max(total, packed.numel()) + P.GUARD_BEHIND <= whole.numel()
    torch.cuda.synchronize()
    codec.pack_batch_device(d.slots, d.desc, d.res, d.n, packed, offs, d.g.max_entry_size if max_entry_size is None else max_entry_size,
                            stream.cuda_stream if stream is not None else None)
    if stream is not None:
        stream.synchronize()                         # that stream only: the call promised to enqueue everything there
    else:
        torch.cuda.synchronize()
    return offs.cpu().numpy().view(np.uint64), whole.cpu().numpy(), lead


def _right(complaints, *where):
    """P.check found nothing; else every complaint in full"""
    assert not complaints, "%r:\n  %s" % (where, "\n  ".join(complaints))


# ---- sizes only ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", P.scan_names())
def test_sizes_only_offsets_are_the_prefix_sum(codec, name):
    """packed = NULL: offsets[0..n] equal the serial sum exactly — across the threads' fours, the waves, the blocks and the trips of the
    block scan, with totals past 2^32 and 2^40, and with failed entries whose comp_size is garbage"""
    import torch
    status, size = P.scan_cases()[name]
    n = len(status)
    res = P.results(status, size)
    ref = P.reference(None, res)
    dres, ddesc, slots = _up(res), _filled(n * zpack_amd.ENCODE_DESC.itemsize, 0), _filled(64, 0)
    for fill in P.FILLS:
        offs = _filled(8 * (n + 1), fill)
        codec.pack_batch_device(slots, ddesc, dres, n, None, offs, int(size.max()))
        torch.cuda.synchronize()
        _right(P.check(ref, offs.cpu().numpy().view(np.uint64), None, 0, fill), (name, fill))
    assert np.array_equal(dres.cpu().numpy().view(zpack_amd.ENCODE_RESULT), res)


def test_no_entries(codec):
    import torch
    dummy = _filled(64, 0)
    for fill in P.FILLS:
        offs = _filled(16, fill)
        codec.pack_batch_device(dummy, dummy, dummy, 0, None, offs, 0)
        torch.cuda.synchronize()
        got = offs.cpu().numpy().view(np.uint64)
        assert int(got[0]) == 0 and got[1:].tobytes() == bytes([fill]) * 8


# ---- gather ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_entry_size", ["tight", "loose"])
@pytest.mark.parametrize("off", [0, 1, 7, 8, 15])
def test_gather_edges(codec, on_device, off, max_entry_size):
    """every length around 16, 64 and PK_SPAN from every slot residue to packed residues of all kinds, the packed base `off` bytes off a
    16-byte boundary; max_entry_size the largest comp_size, and 2^26: it only sizes the launch"""
    d, ref = on_device("edges"), P.gather_reference("edges")
    bound = d.g.max_entry_size if max_entry_size == "tight" else 2**26
    assert d.g.max_entry_size == int(np.where(d.g.res["status"] == 0, d.g.res["comp_size"], 0).max())
    for fill in P.FILLS:
        offs, whole, lead = _pack(codec, d, len(ref.image), fill, off=off, max_entry_size=bound)
        _right(P.check(ref, offs, whole, lead, fill), (off, max_entry_size, fill))
    assert d.slots_unchanged()


@pytest.mark.parametrize("off,max_entry_size", [(0, 48), (9, 48), (5, P.PK_SPAN + 1)])
def test_gather_many(codec, on_device, off, max_entry_size):
    """263 171 entries of 0 to 48 bytes, one in eight failed: the second trip of the size scan and of the span scan, and the binary search
    over a long span_first with runs of entries that have no span"""
    d, ref = on_device("many"), P.gather_reference("many")
    assert d.n > P.TRIP + P.PK_BLOCK
    for fill in P.FILLS:
        offs, whole, lead = _pack(codec, d, len(ref.image), fill, off=off, max_entry_size=max_entry_size)
        _right(P.check(ref, offs, whole, lead, fill), (off, max_entry_size, fill))
    assert d.slots_unchanged()


@pytest.mark.parametrize("which", range(7))
def test_short_buffers(codec, on_device, which):
    """packed_cap = total - k for k in 1, 16, 16383, 16384, 16385, about half of the total, and packed_cap = 0: the offsets are those of
    the whole scan (offsets[n] > packed_cap tells the caller), no byte at or behind packed + packed_cap is written, every entry that ends
    at or in front of the cap is whole, and a byte in front of the cap of the entry that crosses it is its payload's or still the fill"""
    d = on_device("edges")
    total = len(P.gather_reference("edges").image)
    cap = P.short_caps(total)[which]
    ref = P.gather_reference("edges", cap)
    assert 0 <= cap < total == int(ref.offsets[-1])
    for fill in P.FILLS:
        offs, whole, lead = _pack(codec, d, total, fill, off=(3, 0)[which % 2], cap=cap)
        _right(P.check(ref, offs, whole, lead, fill, cap), (cap, fill))
        assert int(offs[-1]) == total
    assert d.slots_unchanged()


def test_gather_on_a_callers_stream(codec, on_device):
    """the same on a stream of the caller's, synchronised on that stream alone"""
    import torch
    d, ref = on_device("edges"), P.gather_reference("edges")
    s = torch.cuda.Stream()
    for fill in P.FILLS:
        offs, whole, lead = _pack(codec, d, len(ref.image), fill, off=3, stream=s)
        _right(P.check(ref, offs, whole, lead, fill), fill)
    assert d.slots_unchanged()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

def test_too_many_entries_are_refused_before_anything_runs(codec):
    """n = 2^31: ZPK_E_INVALID.  pack_launch judges n before it allocates or launches anything (zpk_encode.inc: the test stands in front
    of the scratch's grow), so the arrays handed in are dummies of 64 bytes, and they are as they were."""
    import torch
    for fill in P.FILLS:
        dummy, offs, whole = _filled(64, fill), _filled(64, fill), _filled(P.GUARD_FRONT + P.GUARD_BEHIND, fill)
        for packed in (None, Span(whole.data_ptr() + P.GUARD_FRONT, 16)):
            with pytest.raises(RuntimeError, match=E_INVALID):
                codec.pack_batch_device(dummy, dummy, dummy, 2**31, packed, offs, 16)
        torch.cuda.synchronize()
        for t in (dummy, offs, whole):
            assert (t.cpu().numpy() == fill).all()


def test_a_launch_too_large_is_refused_and_packed_is_untouched(codec):
    """2^20 entries of 8 bytes with max_entry_size = 2^30 would be 2^36 waves: ZPK_E_INVALID, behind the scans (offsets may be written) and
    in front of the gather (packed is not).  The codec is none the worse: the same batch with an honest bound is packed right — 1024 scan
    blocks, four trips of the block scan.  The slots are equal and back to back, so the packed image is the slot image itself."""
    import torch
    n = 2**20
    rng = np.random.default_rng(79)
    slots = np.concatenate([rng.integers(0, 256, 8 * n, dtype=np.uint8), np.full(P.SLOT_PAD, P.GAP_BYTE, dtype=np.uint8)])
    desc = np.zeros(n, dtype=zpack_amd.ENCODE_DESC)
    desc["dst_offset"], desc["dst_capacity"], desc["size"] = np.arange(n, dtype=np.uint64) * np.uint64(8), 8, 8
    res = P.results(np.zeros(n, dtype=np.int32), np.full(n, 8, dtype=np.uint64))
    d = OnDevice(P.Gather("2^20 of 8 bytes", desc, res, slots, 8, None))
    total = 8 * n
    ref = P.Ref(np.arange(n + 1, dtype=np.uint64) * np.uint64(8), slots[:total], np.ones(total, dtype=bool), np.zeros(total, dtype=bool))
    for fill in P.FILLS:
        whole, offs = _filled(P.GUARD_FRONT + total + P.GUARD_BEHIND, fill), _filled(8 * (n + 1), fill)
        with pytest.raises(RuntimeError, match=E_INVALID):
            codec.pack_batch_device(d.slots, d.desc, d.res, n, Span(whole.data_ptr() + P.GUARD_FRONT, total), offs, 2**30)
        torch.cuda.synchronize()
        assert (whole.cpu().numpy() == fill).all()
        offs, image, lead = _pack(codec, d, total, fill, off=1)
        _right(P.check(ref, offs, image, lead, fill), fill)
    assert d.slots_unchanged()


# ---- composition with the encoders ---------------------------------------------------------------------------------------------------

def test_host_path_and_a_direct_call_lay_out_the_same_stream(codec):
    """2 000 small entries, every fifth with dst_capacity = min_capacity - 1, so that it fails in the middle of the batch.
    zpk_codec_encode_batch_host brings every payload home through the scan and the gather: entry i's buffer holds comp_size bytes and
    not one more.  A device encode of the same batch, packed by a direct call: its offsets are the reference's over the HOST path's
    results, and its packed image is the host path's payloads one behind the other."""
    import torch
    n = 2000
    rng = np.random.default_rng(80)
    sizes = rng.integers(1, 3000, n)
    kinds = [(zpack_amd.METHOD_NONE, 0), (zpack_amd.METHOD_ZSTD, 1), (zpack_amd.METHOD_LZ4, 0), (zpack_amd.METHOD_ZSTD, 3)]
    plains = [dg.fill((dg.TEXT, dg.RECORDS, dg.RANDOM)[i % 3], 81, i, int(sizes[i])) for i in range(n)]
    desc = np.zeros(n, dtype=zpack_amd.ENCODE_DESC)
    bound = zpack_amd.lib().zpk_codec_compress_bound
    at_src, at_dst = 0, 5
    for i in range(n):
        m, lv = kinds[i % len(kinds)]
        cap = min_capacity(m, int(sizes[i])) - 1 if i % 5 == 2 else int(bound(m, int(sizes[i])))
        desc[i] = (at_src, int(sizes[i]), at_dst, cap, m, lv)
        at_src += int(sizes[i]) + 16 + i % 3
        at_dst += cap + 1 + i % 16
    blob = np.zeros(at_src + 64, dtype=np.uint8)
    for p, e in zip(plains, desc):
        blob[int(e["src_offset"]):int(e["src_offset"]) + len(p)] = p
    # the host path
    CANARY = 0x6B
    outs = [np.full(int(e["dst_capacity"]) + 8, CANARY, dtype=np.uint8) for e in desc]
    hres = np.zeros(n, dtype=zpack_amd.ENCODE_RESULT)
    sp = (C.c_void_p * n)(*[p.ctypes.data for p in plains])
    dp = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    assert codec.L.zpk_codec_encode_batch_host(codec.h, sp, desc.ctypes.data, n, dp, hres.ctypes.data) == 0
    failed = hres["status"] != 0
    assert np.array_equal(np.nonzero(failed)[0], np.arange(2, n, 5)) and not hres["comp_size"][failed].any()
    for o, k in zip(outs, hres["comp_size"].tolist()):
        assert (o[k:] == CANARY).all()
    ref_offsets = P.reference(None, hres).offsets
    stream = np.concatenate([o[:k] for o, k in zip(outs, hres["comp_size"].tolist())])
    assert len(stream) == int(ref_offsets[-1])
    # a device encode of the same batch, then the call under test
    src, ddesc = _up(blob), _up(desc)
    slots = _filled(at_dst + P.SLOT_PAD, CANARY)
    dres = _filled(n * zpack_amd.ENCODE_RESULT.itemsize, 0)
    codec.encode_batch_device(src, ddesc, n, slots, dres)
    torch.cuda.synchronize()
    res = dres.cpu().numpy().view(zpack_amd.ENCODE_RESULT).copy()
    for f in ("status", "comp_size", "hash"):
        assert np.array_equal(res[f], hres[f]), f
    g = P.Gather("encoded", desc, res, slots.cpu().numpy(), int(desc["dst_capacity"].max()), None)
    ref = P.reference(desc, res, g.slots)
    assert np.array_equal(ref.offsets, ref_offsets) and np.array_equal(ref.image, stream)
    d = OnDevice.__new__(OnDevice)
    d.g, d.n, d.slots, d.desc, d.res = g, n, slots, ddesc, dres
    for fill in P.FILLS:
        offs, whole, lead = _pack(codec, d, len(stream), fill, off=11)
        _right(P.check(ref, offs, whole, lead, fill), fill)
    assert d.slots_unchanged()
