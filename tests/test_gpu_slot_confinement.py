"""include/zpack_codec.h promises that a device decode writes nothing outside [dst_offset, dst_offset + dst_capacity) of an entry, and the
entry points take any dst_offset.  Every other decoder test puts its slots on a 256-byte grid.  Here the same small hand-built inputs —
tests/slot_layouts.py lists them, tests/test_slot_layouts_cpu.py judges them with the oracle alone — are decoded into slots at every
residue of the address: with gaps of 1 to 64 bytes between them, packed back to back, and packed in reverse order, the `dst` pointer
itself odd, guard zones of 4 KiB in front of and behind the image.  Every batch runs all live, and with every second entry refused by
the classification (dst_capacity one short: its whole slot is then a guard directly against its neighbours, which nothing paints over),
and with two fills, so that a stray byte that equals one fill shows under the other.

Asserted of every run: no byte outside a live slot changed; status, produced size, bytes and hash of every live entry are the oracle's;
a refused entry is BUFFER_TOO_SMALL with its slot untouched; every verdict is that of the same batch on the grid; the counters show that
the kernels meant did the work; and the sequence arena of k_zstd_fse holds the oracle's trace for every entry it marks.

NOT asserted: the bytes of a live slot behind the entry's size (the contract leaves them free), which Zstandard entry finishes two-stage
(the arena of an entry is [ceil8(dst_offset), floor8(dst_offset + dst_capacity)), which off the grid can be a record smaller: only the
totals are checked, and printed), and timing.  Guards see writes only: an over-READ next to a slot is invisible to all of this."""
import numpy as np
import pytest

import zpack_amd
from tests import slot_layouts as S
from tests._libs import oracle
from tests.test_gpu_zstd_asm import _arena_bad
from tests.test_zstd_asm_cpu import CAP

pytestmark = pytest.mark.gpu

GROUPS = ("lz4 overlap", "lz4 batches, general, generated", "zstd", "stored") + tuple("lz4 " + d for d in S.DAMAGE) + ("mixed",)
RUNS = [("aligned", None)] + [(layout, which) for layout in S.LAYOUTS[1:] for which in (None, "even", "odd")]


@pytest.fixture(scope="module")
def codec():
    return zpack_amd.Codec(0)


class Batch:
    """one case list: its archive image on the device, and what is computed once and shared — the oracle's verdicts per refusal and
    fill, the oracle's sequence traces, the results of the run on the grid per fill"""

    def __init__(self, cases):
        import torch
        self.cases = cases
        self.arc, self.desc = S.assemble(cases)
        self.src = torch.from_numpy(np.frombuffer(self.arc, dtype=np.uint8).copy()).to(torch.device("cuda:0"))
        self.family = [S.family(c) for c in cases]
        self.labels = ["%s [%s]" % (c["label"], f) for c, f in zip(cases, self.family)]
        self._verdicts, self._control, self._trace = {}, {}, {}

    def verdicts(self, which, fill):
        if (which, fill) not in self._verdicts:
            self._verdicts[which, fill] = S.verdicts(self.arc, self.desc if which is None else S.refuse(self.desc, which), fill)
        return self._verdicts[which, fill]

    def trace(self, i):
        if i not in self._trace:
            self._trace[i] = oracle().zstd_sequences(self.cases[i]["frame"], CAP, 1 << 16)[1]
        return self._trace[i]

    def control(self, codec, fill):
        """the same batch on the 256-byte grid, all live: (results, image, placement)"""
        if fill not in self._control:
            placed = S.lay_out(self.desc["dst_capacity"], "aligned")
            res, image, st = S.run_layout(codec, self.src, S.placed_desc(self.desc, placed), placed, fill)
            self._control[fill] = (res, image, placed, st)
        return self._control[fill]


@pytest.fixture(scope="module")
def batches(golden_dir):
    g = S.groups(golden_dir)
    assert tuple(g) == GROUPS
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Batch(g[name])
        return cache[name]
    return get


def _judge(b, d, res, image, lead, verdicts, fill):
    """every live entry against the oracle — the status; for OK and hash mismatch the produced size, the entry's bytes and the hash — and
    every entry that is not live: BUFFER_TOO_SMALL, nothing produced, its slot (its capacity BEFORE it was refused) still the fill"""
    bad = []
    live = S.is_live(d)
    for i, v in enumerate(verdicts):
        a = lead + int(d[i]["dst_offset"])
        got = (int(res[i]["status"]), int(res[i]["produced"]), int(res[i]["hash"]))
        if got[0] != v.status:
            bad.append((b.labels[i], "status", got[0], "oracle", v.status))
        elif not live[i]:
            if got[:2] != (S.BUFFER_TOO_SMALL, 0) or not (image[a:a + int(b.desc[i]["dst_capacity"])] == fill).all():
                bad.append((b.labels[i], "refused, but", got, "or its slot was written"))
        elif v.status in (S.OK, S.HASH_MISMATCH):
            n = int(d[i]["uncomp_size"])
            if got[1] != v.produced:
                bad.append((b.labels[i], "produced", got[1], "oracle", v.produced))
            elif not np.array_equal(image[a:a + n], v.bytes):
                bad.append((b.labels[i], "first bad byte", int(np.nonzero(image[a:a + n] != v.bytes)[0][0]), "of", n, "slot at", a))
            elif got[2] != v.hash:
                bad.append((b.labels[i], "hash"))
    return bad


def _same_as_on_the_grid(b, d, res, control):
    live = S.is_live(d)
    return [(b.labels[i], "here", res[i], "on the grid", control[i]) for i in range(len(d)) if live[i] and
            (int(res[i]["status"]), int(res[i]["produced"]), int(res[i]["hash"])) != (int(control[i]["status"]), int(control[i]["produced"]), int(control[i]["hash"]))]


def _arena(codec, b, d):
    """(arena words, the oracle's trace) of every live Zstandard entry that k_zstd_fse marked, None for the others"""
    marks = codec.debug_fetch(1, 0, len(d), np.uint32)
    live = S.is_live(d)
    out = []
    for i, c in enumerate(b.cases):
        if c["method"] != S.ZSTD or not live[i] or marks[i] == 0:
            out.append(None)
            continue
        seqs = b.trace(i)
        out.append((codec.debug_fetch(0, (int(d[i]["dst_offset"]) + 7) & ~7, max(1, len(seqs)), np.uint64)[:len(seqs)], seqs))
    return out, marks


@pytest.mark.parametrize("fill", S.FILLS, ids=["fill_a5", "fill_5a"])
@pytest.mark.parametrize("layout,which", RUNS, ids=["%s-%s" % (layout, which or "live") for layout, which in RUNS])
@pytest.mark.parametrize("group", GROUPS)
def test_one_wave_batches_write_only_their_slots(codec, batches, group, layout, which, fill):
    b = batches(group)
    control, _, _, _ = b.control(codec, fill)
    placed = S.lay_out(b.desc["dst_capacity"], layout)
    d = S.placed_desc(b.desc, placed)
    if which:
        d = S.refuse(d, which)
    res, image, st = S.run_layout(codec, b.src, d, placed, fill)
    arena, marks = _arena(codec, b, d)
    live = S.is_live(d)
    on_list = live & (d["comp_size"] > 0)
    lz4 = on_list & (d["method"] == S.LZ4)
    runs = lz4 & (d["comp_size"] < (d["uncomp_size"] >> np.uint64(3)))
    general = [i for i in np.nonzero(lz4 & ~runs)[0] if b.family[i] == "k_lz4_general"]
    nzstd = int((on_list & (d["method"] == S.ZSTD)).sum())
    per_family = {f: sum(1 for i in np.nonzero(on_list)[0] if b.family[i] == f) for f in sorted(set(b.family))}
    print("RECORD %s | %s | %s | fill %#x | live per kernel %s | refused %d | zstd two-stage %d fused %d marked %d | lz4 runs %d general %d handed over %d"
          % (group, layout, which or "all live", fill, per_family, int((~live).sum()), st["zstd_two_stage"], st["zstd_fused"],
             sum(1 for a in arena if a is not None), st["lz4_long_runs"], st["lz4_general"], st["lz4_handed_over"]))
    # 1. nothing outside a live slot
    out = S.outside_untouched(image, placed.lead, d, fill, labels=b.labels)
    assert out == [], ("bytes outside every live slot were written: (index, value, nearest entry [kernel], distance, side)", out[:4])
    # 2., 3. the oracle's verdicts, the refused entries
    assert _judge(b, d, res, image, placed.lead, b.verdicts(which, fill), fill) == []
    # 4. a layout changes no verdict
    assert _same_as_on_the_grid(b, d, res, control) == []
    # 5. not vacuous
    assert (st["fse_watchdog"], st["fse_budget"], st["retried_zstd"], st["retried_lz4"]) == (0, 0, 0, 0), st
    assert st["zstd"] == nzstd and st["zstd_two_stage"] + st["zstd_fused"] == nzstd, (st, nzstd)
    if nzstd:
        assert st["zstd_two_stage"] > 0 and st["zstd_fused"] > 0, st
    assert st["lz4_long_runs"] == int(runs.sum()), (st, int(runs.sum()))
    assert st["lz4"] == int(lz4.sum()) and (st["lz4_general"] > 0) == (len(general) > 0), (st, int(lz4.sum()), len(general))
    assert st["stored"] == int((on_list & (d["method"] == S.NONE)).sum()), st
    # 6. the sequence arena: every marked entry holds the oracle's trace, whoever its neighbours are
    assert _arena_bad(b.cases, arena) == []
    if nzstd:
        assert sum(1 for a in arena if a is not None and len(a[1])) >= nzstd // 3, "too few arenas were compared"


@pytest.mark.parametrize("fill", S.FILLS, ids=["fill_a5", "fill_5a"])
def test_block_parallel_paths_write_only_their_slots(fill):
    """decode_big_batch_device with every entry a candidate (OPT_DEC_SPLIT_MIN 1, OPT_STORED_SPAN_MIN 1): the word stores of k_pj_gather
    and k_zpj_init at addresses that are no multiples of 4, with a partial last word (their first word is whole: a chunk's start is
    counted from the entry, and every frame here is one chunk), and k_stored_span with its first and last words partial (tests/
    slot_layouts.py, big_cases).  An entry goes block-parallel only where that is worth a
    turn of the whole chip, which in a batch it is not: every entry is a call of its own, at ITS place in the gapped layout of the whole
    list, every other slot of the layout a guard."""
    cases = S.big_cases()
    arc, desc = S.assemble(cases)
    placed, grid = S.lay_out(desc["dst_capacity"], "gapped", cover=False), S.lay_out(desc["dst_capacity"], "aligned")
    d, dg = S.placed_desc(desc, placed), S.placed_desc(desc, grid)
    labels = [c["label"] for c in cases]
    codec = zpack_amd.Codec(0)                                               # (options of its own: nothing to put back in another test's codec)
    bad, parallel = [], {}
    try:
        codec.set_option(zpack_amd.OPT_DEC_SPLIT_MIN, 1)
        codec.set_option(zpack_amd.OPT_STORED_SPAN_MIN, 1)       # (the least value; the least entry taken is 1025 bytes, stored_plan.h)
        want = S.verdicts(arc, desc, fill)
        for i, c in enumerate(cases):
            res, image, st = S.run_layout(codec, arc, d[i:i + 1], placed, fill, call="big")
            ctl, _, _ = S.run_layout(codec, arc, dg[i:i + 1], grid, fill, call="big")
            a, n, v = placed.lead + int(d[i]["dst_offset"]), c["uncomp"], want[i]
            got = (int(res[0]["status"]), int(res[0]["produced"]), int(res[0]["hash"]))
            parallel[c["label"]] = (st["device_walked"], st["device_walk_accepted"], st["frame_parallel_entries"], st["stored_span_entries"])
            print("RECORD block-parallel | gapped | fill %#x | %s | slot at %d (mod 4: %d), ends mod 4: %d | walked, accepted, block-parallel, span: %s"
                  % (fill, c["label"][:60], a, a % 4, (a + c["cap"]) % 4, parallel[c["label"]]))
            out = S.outside_untouched(image, placed.lead, d[i:i + 1], fill, labels=labels[i:i + 1])
            if out:
                bad.append((c["label"], "bytes outside the slot", out[:4]))
            if got[0] != v.status or (v.status in (S.OK, S.HASH_MISMATCH) and (got[1:] != (v.produced, v.hash) or not np.array_equal(image[a:a + n], v.bytes))):
                bad.append((c["label"], "here", got, "oracle", v[:3]))
            if got != (int(ctl[0]["status"]), int(ctl[0]["produced"]), int(ctl[0]["hash"])):
                bad.append((c["label"], "here", got, "on the grid", ctl[0]))
            if (st["fse_watchdog"], st["fse_budget"]) != (0, 0):
                bad.append((c["label"], st))
    finally:
        codec.set_option(zpack_amd.OPT_DEC_SPLIT_MIN, 256 << 10)          # (the defaults: dec_plan.h, zpk_codec.hip)
        codec.set_option(zpack_amd.OPT_STORED_SPAN_MIN, 256 << 10)
        codec.close()
    assert bad == []
    # not vacuous: the stored entry went chip-wide, every compressed entry was walked on the device, the four-block LZ4 frame and at
    # least one Zstandard frame were decoded block-parallel (their slots begin and end inside a word: tests/test_slot_layouts_cpu.py)
    assert parallel["stored 1025 bytes"] == (0, 0, 0, 1), parallel
    assert all(p[0] == 1 for label, p in parallel.items() if label != "stored 1025 bytes"), parallel
    assert parallel["lz4 text %d bytes" % (3 * 65536 + 1)][1:3] == (1, 1) and parallel["lz4 text %d bytes" % (65536 + 5)][1:3] == (0, 0), parallel
    assert sum(parallel[c["label"]][2] for c in cases if c["method"] == S.ZSTD and c["label"] in S.BIG_WHOLE_CHIP) >= 1, parallel
