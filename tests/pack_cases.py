"""zpk_codec_pack_batch_device alone: the reference, the inputs and the checker of tests/test_pack_cases_cpu.py (all of this on the
CPU) and tests/test_gpu_pack_alone.py (the device).  Not a test module.  Plain numpy; nothing here needs a GPU.

The call takes `results` and `desc` as plain arrays, so a test writes them itself: no encoder stands between a case and the scan.

  reference(desc, res, slots_image, packed_cap)   offsets = the serial `write_offset += comp_size` over the entries with status 0,
                                                  the packed image by one copy per entry, and for a short buffer which bytes MUST be
                                                  written and which MAY be
  scan_cases()                                    (status, comp_size) for calls without a packed buffer: a comp_size of 2^40 needs no
                                                  memory behind it
  gather_cases()                                  two batches with their slot images: "edges" and "many"
  check(...)                                      what a call left behind against the reference -> a list of complaints, [] = right

Geometry of the kernels under test (zpack_amd/csrc/zpk_encode.inc): a thread scans FOUR entries, a wave 256, a workgroup PK_BLOCK =
1024; k_pack_scan_blocks scans 256 block totals per trip of its loop, so its second trip begins at entry 262 144; the gather copies
PK_SPAN = 16 384 bytes per wave, 16 bytes per lane."""
import collections
import functools

import numpy as np

import zpack_amd

PK_BLOCK = 1024
PK_SPAN = 16384
TRIP = 256 * PK_BLOCK                   # entries per trip of k_pack_scan_blocks' loop
GUARD_FRONT = 4096
GUARD_BEHIND = 65536                    # more than one span: a gather that ignores the cap stays inside the allocation
FILLS = (0xA5, 0x5A)
GAP_BYTE = 0xC3                         # between the slots: neither fill, so a copy from the wrong place shows under both
SLOT_PAD = 64                           # behind the last slot of an image

SCAN_N = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, TRIP, TRIP + 1, 263171)
SPIKES = (2**32 - 1, 2**32, 2**32 + 1, 2**40 + 7)
# the last and the first entry of a thread's four, of a wave, of a block and of a trip of the block scan
SPIKE_AT = (3, 4, 255, 256, PK_BLOCK - 1, PK_BLOCK, TRIP - 1, TRIP)
HOLE_RUNS = (4, 64, 256, PK_BLOCK + 5)
FAIL_STATUS = (12, 14, -1, 1, 0x7FFFFFFF)

EDGE_SIZES = (0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 16383, 16384, 16385, 32767, 32768, 32769,
              3 * 16384 + 5, 2**20 + 3)
MANY_N = 263171
MANY_MAX = 48

Ref = collections.namedtuple("Ref", "offsets image must may")
Gather = collections.namedtuple("Gather", "name desc res slots max_entry_size slot_residue")


def results(status, comp_size):
    r = np.zeros(len(status), dtype=zpack_amd.ENCODE_RESULT)
    r["status"] = status
    r["comp_size"] = comp_size
    r["detail"] = 0xDEAD                           # nothing reads these two
    r["hash"] = 0x0123456789ABCDEF
    return r


def reference(desc, res, slots_image=None, packed_cap=None):
    """-> Ref(offsets[0..n] uint64, packed image | None, must | None, may | None).
    offsets: the exclusive prefix sum of comp_size over the entries with status 0; a failed entry takes no room.
    image: offsets[n] bytes, entry i copied from slots_image[dst_offset : dst_offset + comp_size].
    With packed_cap, two masks over the image: `must` = every byte of every entry that ENDS at or in front of packed_cap; `may` = the
    bytes in front of packed_cap of an entry that crosses it (the kernel drops whole 16 KiB spans of such an entry, and the contract does
    not say which: each of these bytes is the payload's or still the fill).  A byte at or behind packed_cap is in neither."""
    res = np.asarray(res)
    n = len(res)
    size = np.where(res["status"] == 0, res["comp_size"], 0).astype(np.uint64)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(size, out=offsets[1:])
    if slots_image is None:
        return Ref(offsets, None, None, None)
    total = int(offsets[n])
    image = np.zeros(total, dtype=np.uint8)
    cap = total if packed_cap is None else int(packed_cap)
    must = np.zeros(total, dtype=bool)
    may = np.zeros(total, dtype=bool)
    at = desc["dst_offset"].tolist()
    off = offsets.tolist()
    for i in np.nonzero(size)[0].tolist():
        a, b = off[i], off[i + 1]
        assert at[i] + (b - a) <= len(slots_image), (i, "the entry's payload leaves the slot image")
        image[a:b] = slots_image[at[i]:at[i] + (b - a)]
        if b <= cap:
            must[a:b] = True
        elif a < cap:
            may[a:cap] = True
    return Ref(offsets, image, must, may)


def check(ref, got_offsets, whole, lead, fill, packed_cap=None, limit=8):
    """What a call left behind -> complaints.  `whole` is the whole allocation as the device left it, filled with `fill` before the call;
    the packed base is byte `lead` of it.  The offsets are the reference's (also with a short buffer: offsets[n] tells the caller); every
    `must` byte is the payload's, every `may` byte the payload's or the fill; every other byte of the allocation — the guard in front,
    everything at or behind packed_cap, everything behind offsets[n] — is still the fill."""
    out = []
    got_offsets = np.asarray(got_offsets).view(np.uint64)
    if got_offsets.shape != ref.offsets.shape:
        return ["offsets: %d values, not %d" % (len(got_offsets), len(ref.offsets))]
    bad = np.nonzero(got_offsets != ref.offsets)[0]
    if bad.size:
        i = int(bad[0])
        out.append("offsets: %d of %d differ, the first at entry %d (block %d, thread %d, lane %d): %d, not %d" % (
            bad.size, len(ref.offsets), i, i // PK_BLOCK, (i % PK_BLOCK) // 4, ((i % PK_BLOCK) // 4) % 64, int(got_offsets[i]), int(ref.offsets[i])))
    if whole is None:
        return out
    whole = np.asarray(whole)
    total = len(ref.image)
    cap = total if packed_cap is None else int(packed_cap)
    assert lead + max(total, cap) <= len(whole), "the allocation holds the whole packed stream whatever the cap is"
    got = whole[lead:lead + total]
    want_any = ref.must | ref.may
    assert not want_any[min(cap, total):].any() and want_any[:min(cap, total)].all()
    wrong = ref.must & (got != ref.image)
    wrong |= ref.may & (got != ref.image) & (got != fill)
    outside = np.ones(len(whole), dtype=bool)
    outside[lead:lead + total] = ~want_any
    stray = np.nonzero(outside & (whole != fill))[0]
    ends = ref.offsets[1:]
    for k in np.nonzero(wrong)[0][:limit].tolist():
        e = int(np.searchsorted(ends, k, side="right"))
        out.append("packed byte %d (entry %d, its byte %d%s): 0x%02x, not 0x%02x" % (
            k, e, k - int(ref.offsets[e]), ", may stay the fill" if ref.may[k] else "", int(got[k]), int(ref.image[k])))
    if wrong.sum() > limit:
        out.append("... %d packed bytes wrong in all" % int(wrong.sum()))
    for k in stray[:limit].tolist():
        where = ("front guard, %d in front of the base" % (lead - k) if k < lead else
                 "%d behind offsets[n]" % (k - lead - total) if k >= lead + total else "at packed + %d, which is at or behind the cap %d" % (k - lead, cap))
        out.append("byte %d of the allocation was written (0x%02x): %s" % (k, int(whole[k]), where))
    if stray.size > limit:
        out.append("... %d stray bytes in all" % int(stray.size))
    return out


# ---- sizes only ----------------------------------------------------------------------------------------------------------------------

def hole_runs(n):
    """[(first, length)] of the runs of failed entries in the "holes" fill of n entries: the first and the last entry, single ones, and
    runs of 4, 64, 256 and 1024 + 5 beginning on a block boundary and off one — the last of these covers the last five entries of a
    block and the whole next block — and one run of 64 across the boundary of the block scan's trips.  Runs that do not fit are left out."""
    B = PK_BLOCK
    runs = [(0, 1), (n - 1, 1), (7, 1), (100, 1), (B + 476, 1),
            (2 * B, 4), (3 * B + 3, 4), (4 * B, 64), (5 * B + 33, 64), (8 * B, 256), (10 * B + 200, 256),
            (16 * B, B + 5), (20 * B + B - 5, B + 5), (TRIP - 32, 64),
            # below 17 blocks: the same lengths again where a short batch has room for them
            (16, 4), (33, 4), (64, 64), (200, 64), (256, 256), (601, 256)]
    out = []
    for a, k in runs:                  # (a run is kept apart from those taken before it by at least one live entry)
        if a >= 0 and a + k <= n and all(a + k < x or x + j < a for x, j in out):
            out.append((a, k))
    return sorted(out)


def _scan_fill(kind, n, seed):
    rng = np.random.default_rng(seed)
    status = np.zeros(n, dtype=np.int32)
    size = rng.integers(0, 4097, n).astype(np.uint64)
    if kind == "spikes":
        for k, i in enumerate(x for x in SPIKE_AT + (0, n - 1) if x < n):
            size[i] = SPIKES[(k + n) % len(SPIKES)]
    elif kind == "holes":
        for a, k in hole_runs(n):
            status[a:a + k] = [FAIL_STATUS[(a + j) % len(FAIL_STATUS)] for j in range(k)]
            size[a:a + k] = rng.integers(1, 2**44, k)            # garbage: a scan that counts it is far off
    elif kind == "all failed":
        status[:] = [FAIL_STATUS[j % len(FAIL_STATUS)] for j in range(n)]
        size[:] = rng.integers(1, 2**44, n)
    else:
        assert kind == "small", kind
    return status, size


SCAN_KINDS = ("small", "spikes", "holes", "all failed")


def scan_names():
    """the keys of scan_cases(), without building them (a test module's parameter list)"""
    return ["n = %d, %s" % (n, kind) for n in SCAN_N for kind in SCAN_KINDS]


@functools.lru_cache(maxsize=None)
def scan_cases():
    """-> OrderedDict name -> (status int32[n], comp_size uint64[n]), read only.  Every n of SCAN_N with four fills: "small" (0..4096, all
    status 0), "spikes" (one of SPIKES at each index of SPIKE_AT that the batch has, at its first and at its last entry), "holes" (failed
    entries with a garbage comp_size, hole_runs) and "all failed"."""
    out = collections.OrderedDict()
    for n in SCAN_N:
        for k, kind in enumerate(SCAN_KINDS):
            st, sz = _scan_fill(kind, n, 1000 * k + n % 997)
            assert int(np.where(st == 0, sz, 0).astype(object).sum()) < 2**60
            st.setflags(write=False)
            sz.setflags(write=False)
            out["n = %d, %s" % (n, kind)] = (st, sz)
    assert list(out) == scan_names()
    return out


# ---- gather ------------------------------------------------------------------------------------------------------------------------------

def residue_pairs(g):
    """{packed residue: set of slot residues} over the live entries with bytes of a gather case (both mod 16)"""
    off = reference(g.desc, g.res).offsets
    pairs = collections.defaultdict(set)
    for i in np.nonzero((g.res["status"] == 0) & (g.res["comp_size"] > 0))[0].tolist():
        pairs[int(off[i]) % 16].add(int(g.desc["dst_offset"][i]) % 16)
    return pairs


def _edges():
    rng = np.random.default_rng(77)
    live = [(s, r) for s in EDGE_SIZES for r in range(16)]
    order = rng.permutation(len(live)).tolist()
    # (cap, slot residue, status, comp_size): two empty entries, the sizes at every slot residue in a fixed shuffled order, two empty
    # entries; whenever the index is 6 mod 7 a failed entry with a slot of its own and a garbage comp_size no larger than that slot
    rows = []

    def put(cap, residue):
        if len(rows) % 7 == 6:
            fcap = EDGE_SIZES[1 + len(rows) % (len(EDGE_SIZES) - 2)]                   # (1 .. 3 * 16384 + 5)
            rows.append((fcap, int(rng.integers(0, 16)), FAIL_STATUS[len(rows) % len(FAIL_STATUS)], int(rng.integers(1, fcap + 1))))
        rows.append((cap, residue, 0, cap))
    put(0, 5), put(0, 5)
    for k in order:
        put(*live[k])
    put(0, 9), put(0, 9)
    n = len(rows)
    desc = np.zeros(n, dtype=zpack_amd.ENCODE_DESC)
    at, parts = 0, []
    for i, (cap, residue, status, size) in enumerate(rows):
        start = at + 1 + ((residue - (at + 1)) % 16)                  # at least one byte of gap, then the residue asked for
        parts.append(np.full(start - at, GAP_BYTE, dtype=np.uint8))
        parts.append(rng.integers(0, 256, cap, dtype=np.uint8))
        desc[i]["dst_offset"], desc[i]["dst_capacity"], desc[i]["size"] = start, cap, cap
        at = start + cap
    parts.append(np.full(SLOT_PAD, GAP_BYTE, dtype=np.uint8))
    slots = np.concatenate(parts)
    res = results([r[2] for r in rows], [r[3] for r in rows])
    return Gather("edges", desc, res, slots, max(EDGE_SIZES), [r[1] for r in rows])


def _many():
    rng = np.random.default_rng(78)
    n = MANY_N
    cap = rng.integers(0, MANY_MAX + 1, n).astype(np.uint64)
    failed = rng.integers(0, 8, n) == 0
    size = np.where(failed, (rng.random(n) * (cap + np.uint64(1))).astype(np.uint64), cap)   # garbage no larger than the slot
    start = np.cumsum(cap + rng.integers(0, 4, n).astype(np.uint64)) - cap                   # slots 0 to 3 bytes apart
    desc = np.zeros(n, dtype=zpack_amd.ENCODE_DESC)
    desc["dst_offset"], desc["dst_capacity"], desc["size"] = start, cap, cap
    slots = np.full(int(start[-1] + cap[-1]) + SLOT_PAD, GAP_BYTE, dtype=np.uint8)
    inside = np.zeros(len(slots) + 1, dtype=np.int32)
    np.add.at(inside, start.astype(np.int64), 1)
    np.add.at(inside, (start + cap).astype(np.int64), -1)
    inside = np.cumsum(inside[:-1]) > 0
    slots[inside] = rng.integers(0, 256, int(inside.sum()), dtype=np.uint8)
    status = np.where(failed, np.array(FAIL_STATUS, dtype=np.int64)[np.arange(n) % len(FAIL_STATUS)], 0).astype(np.int32)
    return Gather("many", desc, results(status, size), slots, MANY_MAX, (start % np.uint64(16)).astype(np.int64).tolist())


@functools.lru_cache(maxsize=None)
def gather_cases():
    """-> {"edges": Gather, "many": Gather}, read only.
    edges  every size of EDGE_SIZES in a slot at every residue 0..15 mod 16, in an order in which every residue of the PACKED address
           meets at least four residues of the slot address (asserted); at every index that is 6 mod 7 a failed entry with a garbage
           comp_size no larger than its slot; two empty entries side by side at the front and at the end; random bytes in the slots,
           GAP_BYTE between them.
    many   263 171 entries of 0 to 48 bytes, one in eight failed, slots 0 to 3 bytes apart: the second trip of both scans, and the
           gather's binary search over a long span_first with runs of entries that have no span."""
    e, m = _edges(), _many()
    for g in (e, m):
        for a in (g.desc, g.res, g.slots):
            a.setflags(write=False)
        live = g.res["status"] == 0
        assert (g.res["comp_size"] <= g.desc["dst_capacity"]).all(), "no comp_size, garbage included, is larger than its slot"
        assert int((g.desc["dst_offset"] + g.desc["dst_capacity"]).max()) + SLOT_PAD <= len(g.slots)
        assert (g.res["comp_size"][~live] > 0).any()
    pairs = residue_pairs(e)
    assert sorted(pairs) == list(range(16)) and all(len(v) >= 4 for v in pairs.values()), pairs
    assert (e.res["status"][6::7] != 0).all() and (e.res["status"] != 0).sum() == len(e.res[6::7])
    return {"edges": e, "many": m}


@functools.lru_cache(maxsize=None)
def _full_reference(name):
    g = gather_cases()[name]
    r = reference(g.desc, g.res, g.slots)
    for a in r:
        a.setflags(write=False)
    return r


def gather_reference(name, packed_cap=None):
    """the reference of a gather case: computed once and shared where the buffer is whole, afresh for a short one (its masks differ)"""
    if packed_cap is None:
        return _full_reference(name)
    g = gather_cases()[name]
    return reference(g.desc, g.res, g.slots, packed_cap)


def short_caps(total):
    """the short buffers of "edges": total - k for k around a span, about half, and no room at all"""
    return [total - k for k in (1, 16, PK_SPAN - 1, PK_SPAN, PK_SPAN + 1)] + [total // 2 + 3, 0]
