"""The one-wave encoders (k_encode<12|13|14> of zpack_amd/csrc/zpk_encode.inc) in slots of EXACTLY the size they demand, on inputs
whose compressed attempt lands within a few bytes of the block's size on either side, at every small size and every kernel
instantiation — and the frame-format rules no decoder checks (tests/lz4_frames.py).

Everything goes through zpk_codec_encode_batch_device with OPT_ENC_SPLIT_MIN at its default.  One batch of inputs (`build_inputs()`: groups S,
N, L, Q, P) is encoded five times by a module-scoped fixture:

  run A   dst_capacity = zpk_codec_compress_bound; slots at every residue of dst_offset mod 16 in {0, 1, 7, 8, 15}, >= 512 bytes of
          canary between them and 4096 behind the last
  run B   dst_capacity = min_capacity(method, len) (tests/test_enc_capacity_cpu.py), the same slot offsets
  run C   min_capacity - 1 for every third entry
  run D   the slots of run B packed back to back with no gap
  run E   groups S and N at the minimum through zpk_codec_encode_batch_host

An overrun of a few hundred bytes lands in a canary region inside the allocation: a finding, never a fault.  The tests only read what
the fixture left."""
import time

import numpy as np
import pytest

import zpack_amd
from benchdata import datagen as dg
from tests import lz4_frames, zpk
from tests._libs import oracle, have_ref, ref
from tests.test_enc_capacity_cpu import min_capacity
from tests.test_gpu_big_encode_device import Batch, CANARY, R_BUFFER_TOO_SMALL, R_COMPRESS_FAILED, _home, _same_results
from zpack_amd import METHOD_NONE, METHOD_ZSTD, METHOD_LZ4

pytestmark = pytest.mark.gpu
GAP, TAIL, FRONT = 512, 4096, 1024
RESIDUES = (0, 1, 7, 8, 15)
BLOCK = 65536

S_LENGTHS = (0, 1, 2, 3, 4, 5, 11, 12, 13, 14, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096,
             65535, 65536, 65537, 65536 + 255, 65536 + 256, 65536 + 257, 131072, 131073)
S_METHODS = ((METHOD_LZ4, 0), (METHOD_LZ4, 3), (METHOD_LZ4, 9), (METHOD_ZSTD, 1), (METHOD_ZSTD, 3), (METHOD_ZSTD, 9), (METHOD_NONE, 0))
# Group N.  `k` copies of `ml` bytes are planted in the last `n` (or, for 65536 + 4096, the last 4096) bytes of a random entry: the
# last block's compressed size falls by a few bytes per copy and crosses its plain size somewhere in the sweep.  Where: measured on the
# CPU with the oracle's LZ4 encoder on these very inputs (first k at which the last block goes out compressed, in brackets the
# differences plain - compressed over the five k from there): see N_SWEEP.  The device's parse differs (it misses a copy whose
# hash-table slot was overwritten), so the sweeps are ~40 wide; the Zstandard writer needs its 16-byte margin and ~3.3 bytes per
# sequence whatever the block's size, so its crossing sits at a small k for every n.
N_LAST = {4096: 4096, 8192: 8192, 65536: 65536, 65536 + 4096: 4096}       # entry length -> length of its last block
N_SWEEP = {}                                                              # (method, n, ml) -> range of k; filled below
L_RUNS = (14, 15, 16, 31, 32, 33, 255, 256, 257, 15 + 254, 15 + 255, 15 + 256, 15 + 2 * 255)
L_MATCHES = (18, 19, 20, 19 + 254, 19 + 255, 19 + 256)
Q_COUNTS = tuple(range(50, 69)) + tuple(range(100, 133))      # (the parse cuts some copies in two: 60 planted gave 64 sequences, 124 gave 153)
P_PERIODS = (65535, 65536, 65537)


def _random(seed, n):
    return np.random.RandomState(seed).randint(0, 256, n).astype(np.uint8)


def plant(seed, n, k, ml, region=None):
    """n random bytes; k copies of ml bytes, one in each k-th of what lies behind byte 1024 of the last `region` bytes (default: of all n), each taken
    from 600 to 1600 bytes further up in that region (the match finder looks candidates up 256 positions at a time, and a slot of
    k_encode<12>'s table of 4096 survives ~1000 positions three times out of four) and fenced by bytes that differ from the source's
    neighbours, so that the planted length is the match's."""
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, n).astype(np.uint8)
    base = 0 if region is None else n - region                             # where the block the copies lie in begins
    lo = base + 1024
    span = n - 32 - lo
    assert k * (ml + 4) <= span, (n, k, ml)
    for j in range(k):
        d = lo + j * (span // k) + 1 + int(rng.randint(0, span // k - ml - 2))   # (jittered: evenly spaced runs would all change their length bytes at one k)
        s = int(rng.randint(max(base + 1, d - 1600), d - 600))
        a[d:d + ml] = a[s:s + ml]
        if a[d - 1] == a[s - 1]:
            a[d - 1] ^= 0x55
        if a[d + ml] == a[s + ml]:
            a[d + ml] ^= 0x55
    return a


def ruler(seed, run, ml):
    """A pool of random bytes, then three times (`run` random literals, a copy of `ml` bytes out of the pool), then 20 literals: the
    second and third sequence have exactly `run` literals and all three matches exactly `ml` bytes, if the parse finds them."""
    rng = np.random.RandomState(seed)
    pool = max(700, 32 + 3 * (ml + 8))
    parts = [rng.randint(0, 256, pool).astype(np.uint8)]
    for i in range(3):
        s = 16 + i * (ml + 8)
        lits = rng.randint(0, 256, run).astype(np.uint8)
        if lits[-1] == parts[0][s - 1]:
            lits[-1] ^= 0x55
        parts += [lits, parts[0][s:s + ml].copy()]
    tail = rng.randint(0, 256, 20).astype(np.uint8)
    out = np.concatenate(parts + [tail])
    # the byte behind every copy differs from the byte behind its source
    at = pool
    for i in range(3):
        s = 16 + i * (ml + 8)
        at += run + ml
        if out[at] == out[s + ml]:
            out[at] ^= 0x55
    return out


def _pattern(period, n, seed):
    unit = _random(seed, period) if period > 1 else np.array([0x5A], dtype=np.uint8)
    return np.resize(unit, n).astype(np.uint8) if n else np.zeros(0, dtype=np.uint8)


def n_inputs(n, ml, ks):
    return [(k, plant(7000 + n % 1000 + ml, n, k, ml, region=N_LAST[n] if N_LAST[n] != n else None)) for k in ks]


# (method, entry length, ml) -> the k swept, step 1.  First k at which the ORACLE's LZ4 encoder compresses the last block of these inputs:
# (4096, 5) 13, (4096, 8) 4, (8192, 5) 24, (8192, 8) 8, (65536, 5) 180, (65536, 8) 60, (65536 + 4096, 5) 13, (65536 + 4096, 8) 6, with
# plain - compressed = 4 4 4 6 11 / 2 5 10 14 15 / 1 2 1 5 9 / 2 4 13 16 20 / 3 3 9 14 (steps of 4) / 6 26 44 52 (steps of 4) / 3 3 4 8 8 /
# 10 13 14 20 26 from there.  The device's first compressed k, measured on an MI355X, in the same order: LZ4 level 0 13, 4, 28, 8, 185
# (stored again up to 205), 61, 13, 6; Zstandard level 1 17, 5, 27, 6, 40, 8, 18, 6 and level 3 17, 5, 23, 6, 35, 6, 17, 6.
for _n in N_LAST:
    for _ml in (5, 8):
        N_SWEEP[(METHOD_LZ4, _n, _ml)] = range(0, 44)
        N_SWEEP[(METHOD_ZSTD, _n, _ml)] = range(0, 44)
N_SWEEP[(METHOD_LZ4, 8192, 5)] = range(10, 54)
N_SWEEP[(METHOD_LZ4, 65536, 5)] = range(170, 214)
N_SWEEP[(METHOD_LZ4, 65536, 8)] = range(44, 88)
N_SWEEP[(METHOD_ZSTD, 65536, 5)] = range(16, 60)


class Entry:
    def __init__(self, group, tag, plain, method, level, last=None):
        self.group, self.tag, self.plain, self.method, self.level = group, tag, plain, method, level
        self.last = last                                                   # group N: the plain length of the last block

    def __repr__(self):
        return "%s %s len %d method %d level %d" % (self.group, self.tag, len(self.plain), self.method, self.level)


def build_inputs():
    E = []
    # S: sizes x content x every kernel instantiation.  Above 4096: constant, one pattern, text, random (stored: constant and random)
    for li, n in enumerate(S_LENGTHS):
        contents = [("const", _pattern(1, n, 0)), ("random", dg.fill(dg.RANDOM, 1501, li, n)), ("text", dg.fill(dg.TEXT, 1500, li, n)),
                    ("period3", _pattern(3, n, 33))]
        if n <= 4096:
            contents += [("period%d" % p, _pattern(p, n, 30 + p)) for p in (2, 4, 5)]
        for name, plain in contents:
            for m, lv in S_METHODS:
                if m == METHOD_NONE and name not in ("const", "random"):
                    continue
                E.append(Entry("S", name, plain, m, lv))
    # N: near-misses
    for (m, n, ml), ks in sorted(N_SWEEP.items()):
        for k, plain in n_inputs(n, ml, ks):
            for lv in ((0,) if m == METHOD_LZ4 else (1, 3)):
                E.append(Entry("N", (n, ml, k), plain, m, lv, last=N_LAST[n]))
    # L: length rulers
    for ri, run in enumerate(L_RUNS):
        for mi, ml in enumerate(L_MATCHES):
            plain = ruler(8000 + 16 * ri + mi, run, ml)
            for m, lv in ((METHOD_LZ4, 0), (METHOD_LZ4, 3), (METHOD_LZ4, 9), (METHOD_ZSTD, 1), (METHOD_ZSTD, 3)):
                E.append(Entry("L", (run, ml), plain, m, lv))
    # Q: sequence counts around ZE_FSE_MIN_SEQ = 64 and the Number_of_Sequences forms at 128
    for k in Q_COUNTS:
        plain = plant(9000 + k, 16384, k, 64)
        for m, lv in ((METHOD_ZSTD, 1), (METHOD_ZSTD, 3), (METHOD_LZ4, 0)):
            E.append(Entry("Q", k, plain, m, lv))
    # P: later blocks repeat the first at a period of 65535 (the furthest an LZ4 offset reaches), 65536 and 65537
    for period in P_PERIODS:
        unit = _random(9500 + period, period)
        for n in (2 * BLOCK, 2 * BLOCK + 5000):
            plain = np.resize(unit, n)
            for m, lv in ((METHOD_LZ4, 0), (METHOD_LZ4, 9), (METHOD_ZSTD, 1), (METHOD_ZSTD, 3)):
                E.append(Entry("P", (period, n), plain, m, lv))
    return E


def bounds(E):
    b = zpack_amd.lib().zpk_codec_compress_bound
    return [int(b(e.method, len(e.plain))) for e in E]


def minimums(E):
    return [min_capacity(e.method, len(e.plain)) for e in E]


def spread_offsets(E):
    """slot i starts at a residue of RESIDUES[i % 5] mod 16, at least GAP bytes behind the end of slot i - 1's BOUND"""
    offs, at = [], FRONT
    for i, full in enumerate(bounds(E)):
        at = ((at + 15) & ~15) + RESIDUES[i % len(RESIDUES)]
        offs.append(at)
        at += full + GAP
    return offs


def packed_offsets(E):
    caps = minimums(E)
    return [FRONT + 7 + int(x) for x in np.concatenate([[0], np.cumsum(caps)[:-1]])]


def make_batch(E, caps, offsets):
    return Batch([e.plain for e in E], [(e.method, e.level) for e in E], caps=caps, dst_offsets=offsets, tail=TAIL)


def payload(image, desc, res, i):
    a = int(desc["dst_offset"][i])
    return image[a:a + int(res["comp_size"][i])]


def canary_intact(image, desc, res):
    """every byte of the allocation outside [dst_offset, dst_offset + comp_size) of every entry is still the canary"""
    mask = np.ones(len(image), dtype=bool)
    for a, k in zip(desc["dst_offset"], res["comp_size"]):
        mask[int(a):int(a) + int(k)] = False
    bad = np.nonzero(mask & (image != CANARY))[0]
    if bad.size:
        starts = np.asarray(desc["dst_offset"], dtype=np.int64)
        order = np.argsort(starts)
        who = order[np.searchsorted(starts[order], bad[:8], side="right") - 1]
        raise AssertionError("%d bytes outside the frames were written; the first at %s, behind the starts of entries %s by %s (capacities %s, comp_size %s)" % (
            bad.size, bad[:8], who, bad[:8] - starts[who], desc["dst_capacity"][who], res["comp_size"][who]))


def zstd_blocks(frame):
    """[(type, Block_Size, bytes in the frame)] of a single-segment frame without checksum, and its Frame_Content_Size"""
    f = bytes(frame)
    assert f[:4] == b"\x28\xb5\x2f\xfd" and f[4] & 0x2F == 0x20, f[:5].hex()
    nf = (1, 2, 4, 8)[f[4] >> 6]
    fcs = int.from_bytes(f[5:5 + nf], "little") + (256 if nf == 2 else 0)
    p, out = 5 + nf, []
    while True:
        bh = int.from_bytes(f[p:p + 3], "little")
        last, typ, size = bh & 1, (bh >> 1) & 3, bh >> 3
        out.append((typ, size, 1 if typ == 1 else size))
        p += 3 + out[-1][2]
        if last:
            break
    assert p == len(f), (p, len(f))
    return out, fcs


# ---- the runs ---------------------------------------------------------------------------------------------------------------------------

class Run:
    def __init__(self, batch, image, res):
        self.batch, self.desc, self.image, self.res = batch, batch.desc, image, res


@pytest.fixture(scope="module")
def codec():
    c = zpack_amd.Codec(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def runs(codec):
    """The inputs, built once with fixed seeds, and runs A to E (see the module's docstring); read only."""
    class R:
        pass
    R.t0 = time.time()
    R.E = E = build_inputs()
    for e in E:
        if e.tag == "random" and len(e.plain) > 1:
            assert (e.plain != e.plain[0]).any()
    R.bound, R.min = bounds(E), minimums(E)
    assert all(b >= m for b, m in zip(R.bound, R.min))
    offs = spread_offsets(E)
    assert {o % 16 for o in offs} == set(RESIDUES) and all(b - (a + cap) >= GAP for a, b, cap in zip(offs, offs[1:], R.bound))

    def go(batch, first=None):
        if first is not None:
            batch.src = first.src                                           # (the same plaintexts at the same source offsets)
        return Run(batch, *_home(*batch.run(codec, call="batch")))
    R.A = go(make_batch(E, None, offs))
    R.B = go(make_batch(E, R.min, offs), R.A.batch)
    R.tight = [i for i in range(0, len(E), 3) if R.min[i] > 0]
    caps_c = list(R.min)
    for i in R.tight:
        caps_c[i] -= 1
    R.C = go(make_batch(E, caps_c, offs), R.A.batch)
    R.C_host = R.C.batch.host(codec)
    R.D = go(make_batch(E, R.min, packed_offsets(E)), R.A.batch)
    R.sn = [i for i, e in enumerate(E) if e.group in "SN"]
    sub = [E[i] for i in R.sn]
    R.E_host = make_batch(sub, minimums(sub), None).host(codec)
    R.t_runs = time.time() - R.t0
    print("\n[encode slots] %d entries, %.1f MB of plaintext, inputs + five runs %.1f s" % (len(E), sum(len(e.plain) for e in E) / 1e6, R.t_runs))
    return R


@pytest.fixture(scope="module")
def walks(runs):
    """lz4_frames.walk over every LZ4 frame of run A: {entry index: blocks}; a frame the walker turns down is left out here and listed
    in runs.walk_errors, for test_lz4_frames_keep_the_format_rules to report"""
    A, out, runs.walk_errors = runs.A, {}, []
    for i, e in enumerate(runs.E):
        if e.method == METHOD_LZ4:
            try:
                out[i] = lz4_frames.walk(payload(A.image, A.desc, A.res, i).tobytes(), len(e.plain))
            except AssertionError as err:
                runs.walk_errors.append((i, e, str(err)))
    return out


@pytest.fixture(scope="module")
def zstats(runs):
    """the oracle's trace and statistics of every Zstandard frame of run A: {entry index: dict}"""
    o, A, out = oracle(), runs.A, {}
    for i, e in enumerate(runs.E):
        if e.method != METHOD_ZSTD:
            continue
        frame = payload(A.image, A.desc, A.res, i).tobytes()
        rc, seqs = o.zstd_sequences(frame, len(e.plain), 1 << 16)
        st = o.zstd_stats()
        assert rc == 0 and len(seqs) == st.sequences < (1 << 16), (i, e, rc)
        out[i] = dict(seqs=seqs, single=st.single_segment, window=int(st.window_size), fcs_bytes=st.fcs_bytes, raw=st.raw_blocks, rle=st.rle_blocks,
                      comp=st.comp_blocks, lit_raw=st.lit_raw, lit_huf=st.lit_huf, modes=[[st.seq_mode[k][m] for m in range(4)] for k in range(3)],
                      nseq_form=list(st.nseq_form), blocks=zstd_blocks(frame))
    return out


def _decode(o, frame, e, h):
    import ctypes as C
    k, n = len(frame), len(e.plain)
    arc = np.zeros(10 + k + 64, dtype=np.uint8)                              # (the entry inside an archive image: the checker has the reader's offset guards)
    arc[10:10 + k] = frame
    out = np.zeros(max(n, 1), dtype=np.uint8)
    got, hh = C.c_uint64(0), C.c_uint64(0)
    u8p = C.POINTER(C.c_uint8)
    rc = o.lib.orc_entry_decode(arc.ctypes.data_as(u8p), len(arc), 10, k, n, h, e.method, out.ctypes.data_as(u8p), n, C.byref(got), C.byref(hh))   # oracle().entry_decode without its copies
    return rc, got.value, out[:n]


# ---- run A ----------------------------------------------------------------------------------------------------------------------------

def test_bound_sized_slots_results_and_canaries(runs):
    """Run A: every status 0, every hash the real XXH3's, comp_size <= capacity, and every byte outside [dst_offset, dst_offset +
    comp_size) of every slot — the unused rest of each slot included — still the canary."""
    A, E = runs.A, runs.E
    assert (A.res["status"] == 0).all(), [(i, E[i], A.res[i]) for i in np.nonzero(A.res["status"])[0][:8]]
    assert [int(h) for h in A.res["hash"]] == [dg.xxh3(e.plain) for e in E]
    assert (A.res["comp_size"] <= A.desc["dst_capacity"]).all()
    canary_intact(A.image, A.desc, A.res)


def test_frames_decode_to_their_plaintexts(runs):
    """Run A: the oracle decodes every frame to its plaintext — and the compiled reference, where it was built.  Incompressible
    entries (dg.RANDOM; stored ones) come out at exactly min_capacity: every block stored, the frame the capacity check assumes."""
    A, E, o = runs.A, runs.E, oracle()
    for i, e in enumerate(E):
        rc, got, out = _decode(o, payload(A.image, A.desc, A.res, i), e, int(A.res["hash"][i]))
        assert rc == 0 and got == len(e.plain) and np.array_equal(out, e.plain), (i, e, rc, got)
    exact = [i for i, e in enumerate(E) if e.group == "S" and (e.tag == "random" or e.method == METHOD_NONE)]
    assert len(exact) >= 7 * len(S_LENGTHS)
    for i in exact:
        assert int(A.res["comp_size"][i]) == runs.min[i], (i, E[i], A.res[i], runs.min[i])
    if have_ref():
        import ctypes as C
        pay, ents, at = [], [], 10
        for i, e in enumerate(E):
            f = payload(A.image, A.desc, A.res, i).tobytes()
            pay.append(f)
            ents.append(("e%d" % i, at, len(f), len(e.plain), int(A.res["hash"][i]), e.method))
            at += len(f)
        R = ref()
        rc, r, keep = R.open_memory(zpk.assemble(pay, ents))
        assert rc == 0
        for i, e in enumerate(E):
            out = np.zeros(max(1, len(e.plain)), dtype=np.uint8)
            rc = R.lib.zpack_read_file(C.byref(r), C.byref(r.file_entries[i]), out.ctypes.data_as(C.POINTER(C.c_uint8)), len(e.plain), None)
            assert rc == 0 and np.array_equal(out[:len(e.plain)], e.plain), (i, e, rc)
        R.close_reader(r)


def test_lz4_frames_keep_the_format_rules(runs, walks):
    """Run A: every LZ4 frame passes the strict walker (tests/lz4_frames.py) — among its rules the end-of-block ones no decoder checks
    and `a compressed block is smaller than its plaintext`.  Both kinds of block were walked, at every level."""
    E = runs.E
    assert not runs.walk_errors, (len(runs.walk_errors), runs.walk_errors[:4])
    for lv in (0, 3, 9):
        mine = [walks[i] for i in walks if E[i].level == lv]
        assert any(b[0] for w in mine for b in w) and any(not b[0] for w in mine for b in w), lv
    for i, w in walks.items():
        assert sum(4 + b[2] for b in w) + 11 == int(runs.A.res["comp_size"][i])
        if len(E[i].plain) < 13:
            assert all(b[0] for b in w)


def test_zstd_frames_headers_windows_and_coverage(runs, zstats):
    """Run A: every Zstandard frame is single-segment with Frame_Content_Size = its length, and no executed offset is larger than the
    window.  Over the batch: RLE, raw and compressed blocks, Frame_Content_Size fields of 1, 2 and 4 bytes (the switches at 256 and
    65536 + 256), raw and Huffman literals, predefined and FSE sequence tables all occur — in every kernel instantiation's entries."""
    E = runs.E
    for i, z in zstats.items():
        n = len(E[i].plain)
        assert z["single"] == 1 and z["window"] == n and z["blocks"][1] == n, (i, E[i], z["window"])
        assert z["fcs_bytes"] == (1 if n < 256 else 2 if n < 65536 + 256 else 4), (i, E[i])
        if len(z["seqs"]):
            assert int((z["seqs"] & np.uint64((1 << 29) - 1)).max()) <= z["window"], (i, E[i])
        kinds = [t for t, _, _ in z["blocks"][0]]
        assert (kinds.count(0), kinds.count(1), kinds.count(2)) == (z["raw"], z["rle"], z["comp"])
        plain = [min(BLOCK, n - at) for at in range(0, max(n, 1), BLOCK)]                     # (a compressed block's header holds its compressed size)
        assert len(kinds) == len(plain) and all(t == 2 and c < p or t < 2 and s == p for (t, s, c), p in zip(z["blocks"][0], plain)), (i, E[i], z["blocks"][0])
    for lv in (1, 3, 9):
        mine = [z for i, z in zstats.items() if E[i].level == lv]
        tot = lambda key: sum(z[key] for z in mine)
        seen = dict(rle=tot("rle"), raw=tot("raw"), comp=tot("comp"), lit_raw=tot("lit_raw"), lit_huf=tot("lit_huf"),
                    predefined=sum(z["modes"][k][0] for z in mine for k in range(3)), fse=sum(z["modes"][k][2] for z in mine for k in range(3)))
        print("[encode slots] Zstandard level %d: %s, fcs_bytes %s" % (lv, seen, sorted({z["fcs_bytes"] for z in mine})))
        assert all(seen.values()), (lv, seen)
        assert {z["fcs_bytes"] for z in mine} == {1, 2, 4}, lv


def test_near_misses_fall_on_both_sides(runs, walks, zstats):
    """Group N, per (method, entry length, planted match length): the sweep holds an entry whose last block was stored and one whose last
    block went out compressed; for LZ4 a compressed last block within 16 bytes of its plain size.  The closest approaches (smallest
    plain - compressed) are printed."""
    E = runs.E
    fam = {}
    for i, e in enumerate(E):
        if e.group != "N":
            continue
        n, ml, k = e.tag
        if e.method == METHOD_LZ4:
            if i not in walks:
                continue
            stored, n_plain, n_comp, _ = walks[i][-1]
        else:
            typ, _, n_comp = zstats[i]["blocks"][0][-1]
            stored, n_plain = typ == 0, e.last
            assert typ in (0, 2)
        assert n_plain == e.last
        fam.setdefault((e.method, e.level, n, ml), []).append((k, stored, n_plain - n_comp))
    assert len(fam) == 8 + 16
    for key, rows in sorted(fam.items()):
        comp = [(d, k) for k, stored, d in rows if not stored]
        st = [k for k, stored, d in rows if stored]
        print("[encode slots] N %s: stored at k %s..%s (%d), compressed at k %s..%s (%d), closest approach %s (plain - compressed, k)" % (
            key, min(st, default=None), max(st, default=None), len(st), min((k for _, k in comp), default=None), max((k for _, k in comp), default=None),
            len(comp), sorted(comp)[:4]))
        assert st and comp, key
        assert min(comp)[0] >= 1
        if key[0] == METHOD_LZ4:
            assert min(comp)[0] <= 16, (key, sorted(comp)[:4])


def test_length_rulers_reach_the_encoders_switches(runs, walks):
    """Group L: over the group's LZ4 frames every listed literal-run length (around 15, 32, ZE_LANE_LIT = 256 and the 255-steps of the
    length bytes) and match length (around 19 and 19 + 255) occurs in a sequence."""
    lls, mls = set(), set()
    for i, w in walks.items():
        if runs.E[i].group == "L":
            for b in w:
                lls.update(s[0] for s in b[3] if s[1])
                mls.update(s[1] for s in b[3] if s[1])
    print("[encode slots] L: literal runs seen %s of %s, match lengths seen %s of %s" % (sorted(lls & set(L_RUNS)), list(L_RUNS), sorted(mls & set(L_MATCHES)), list(L_MATCHES)))
    assert set(L_RUNS) <= lls and set(L_MATCHES) <= mls, (sorted(set(L_RUNS) - lls), sorted(set(L_MATCHES) - mls))


def test_sequence_counts_bracket_64_and_128(runs, zstats):
    """Group Q (one block per entry): blocks with fewer than and with at least ZE_FSE_MIN_SEQ = 64 sequences, fewer than and at least 128
    (the one- and two-byte Number_of_Sequences), at both levels."""
    for lv in (1, 3):
        counts = sorted(len(z["seqs"]) for i, z in zstats.items() if runs.E[i].group == "Q" and runs.E[i].level == lv and z["comp"] == 1)
        forms = [sum(z["nseq_form"][f] for i, z in zstats.items() if runs.E[i].group == "Q" and runs.E[i].level == lv) for f in range(4)]
        print("[encode slots] Q level %d: sequences per block %s, Number_of_Sequences forms %s" % (lv, counts, forms))
        assert counts[0] < 64 and any(64 <= c < 128 for c in counts) and counts[-1] >= 128, counts
        assert 63 in counts or 64 in counts or (max(c for c in counts if c < 64) >= 60 and min(c for c in counts if c >= 64) <= 68)
        assert forms[1] and forms[2], forms


def test_far_offsets(runs, walks, zstats):
    """Group P: random blocks repeated at a period of 65535, 65536 and 65537.  65535 is the furthest an LZ4 offset reaches: the later
    blocks, where the parse still holds a candidate that far back, compress with that offset and no other (at least one entry does);
    one byte further and every block is stored.  (Zstandard: whatever the parse found, no offset
    beyond the window — test_zstd_frames_headers_windows_and_coverage; here what it found is printed.)"""
    E, reached = runs.E, []
    for i, e in enumerate(E):
        if e.group != "P":
            continue
        period = e.tag[0]
        if e.method == METHOD_LZ4 and i in walks:
            w = walks[i]
            if period == 65535:
                assert w[0][0], e
                for b in w[1:]:
                    if not b[0]:
                        reached.append(e)
                        assert {s[2] for s in b[3] if s[1]} == {65535}, (e, b[:3])
            else:
                assert all(b[0] for b in w), (e, [b[:3] for b in w])
        elif e.method == METHOD_ZSTD:
            z = zstats[i]
            offs = sorted({int(x) for x in z["seqs"] & np.uint64((1 << 29) - 1)})
            print("[encode slots] P %s: blocks %s, offsets %s" % (e, [(t, c) for t, _, c in z["blocks"][0]], offs[:6]))
    # (a table slot has to survive 65535 positions: k_encode<12>'s 4096 slots do not, k_encode<14>'s 2 x 16384 do often enough)
    print("[encode slots] P: LZ4 entries with a block compressed at offset 65535: %s" % reached)
    assert reached


# ---- runs B to E ------------------------------------------------------------------------------------------------------------------------

def _same_frames(E, one, other, idx=None):
    for j, i in enumerate(range(len(E)) if idx is None else idx):
        assert np.array_equal(payload(one.image, one.desc, one.res, i), payload(other.image, other.desc, other.res, i)), (i, E[i])


def test_minimum_capacity_changes_no_frame(runs):
    """Run B, dst_capacity = min_capacity for every entry: results and frames identical to run A's, every byte outside the frames still
    the canary.  (The run that shows a margin short by a few bytes: the attempt on the last block has the block's length + 4 (LZ4) or
    + 0 (Zstandard) bytes behind its start.)"""
    A, B = runs.A, runs.B
    assert np.array_equal(B.desc["dst_capacity"], np.array(runs.min, dtype=np.uint64)) and np.array_equal(B.desc["dst_offset"], A.desc["dst_offset"])
    _same_results(B.res, A.res)
    _same_frames(runs.E, B, A)
    canary_intact(B.image, B.desc, B.res)


def test_one_byte_short_fails_before_anything_is_written(runs):
    """Run C, min_capacity - 1 for every third entry: COMPRESS_FAILED (stored: BUFFER_TOO_SMALL) with comp_size = hash = 0 and the
    whole slot still canary; every other entry bit-identical to run B; zpk_codec_encode_batch_host gives the same verdicts."""
    B, Cr, E = runs.B, runs.C, runs.E
    tight = set(runs.tight)
    assert len(tight) >= len(E) // 3 - 8
    for i, e in enumerate(E):
        if i in tight:
            want = R_BUFFER_TOO_SMALL if e.method == METHOD_NONE else R_COMPRESS_FAILED
            assert (int(Cr.res["status"][i]), int(Cr.res["comp_size"][i]), int(Cr.res["hash"][i])) == (want, 0, 0), (i, e, Cr.res[i])
        else:
            assert Cr.res[i] == B.res[i], (i, e)
            assert np.array_equal(payload(Cr.image, Cr.desc, Cr.res, i), payload(B.image, B.desc, B.res, i)), (i, e)
    canary_intact(Cr.image, Cr.desc, Cr.res)
    _same_results(Cr.res, runs.C_host[0])


def test_packed_slots_give_the_same_frames(runs):
    """Run D, the slots of run B back to back in descriptor order: results and frames identical, the canaries in front of the first
    and behind the last slot intact."""
    B, D, E = runs.B, runs.D, runs.E
    d = D.desc
    assert np.array_equal(d["dst_offset"][1:], (d["dst_offset"] + d["dst_capacity"])[:-1])
    _same_results(D.res, B.res)
    _same_frames(E, D, B)
    first, end = int(d["dst_offset"][0]), int(d["dst_offset"][-1] + d["dst_capacity"][-1])
    assert first >= 512 and len(D.image) - end >= TAIL
    assert (D.image[:first] == CANARY).all() and (D.image[end:] == CANARY).all()


def test_host_path_at_minimum_capacity(runs):
    """Run E, groups S and N through zpk_codec_encode_batch_host into host buffers of exactly min_capacity: statuses, sizes, hashes
    and bytes are run B's."""
    B = runs.B
    res, pay = runs.E_host
    _same_results(res, B.res[runs.sn])
    for j, i in enumerate(runs.sn):
        assert np.array_equal(pay[j], payload(B.image, B.desc, B.res, i)), (i, runs.E[i])
