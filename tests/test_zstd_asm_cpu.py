"""The hand-built Zstandard frames of tests/zstd_asm.py before they go near a GPU: libzstd (the library the compiled reference links) and
the oracle must agree on every one of them — valid or not, and every byte — and the oracle's statistics and sequence trace must show that
each frame exercises what its label says.  libzstd decides what is expected; where the oracle disagreed it was the oracle that changed
(a Number_of_Sequences of 0 in the two-byte form, blocks whose lengths add up to more than Block_Maximum_Size)."""
import ctypes as C
import ctypes.util

import numpy as np
import pytest

from tests import zpk
from tests import zstd_asm as Z
from tests._libs import have_ref, oracle, ref

CAP = 1 << 19
STAT_FIELDS = ("blocks", "raw_blocks", "rle_blocks", "comp_blocks", "lit_raw", "lit_rle", "lit_huf", "lit_treeless", "lit_huf_1stream",
               "lit_huf_4stream", "huf_fse_weights", "huf_direct_weights", "sequences", "repcode_uses", "window_size", "single_segment",
               "has_fcs", "has_checksum", "huf_max_bits")


@pytest.fixture(scope="module")
def libzstd():
    z = C.CDLL(ctypes.util.find_library("zstd"))
    z.ZSTD_decompress.restype = C.c_size_t
    z.ZSTD_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    z.ZSTD_isError.argtypes = [C.c_size_t]
    return z


def _unpack(v):
    v = int(v)
    return v & ((1 << 29) - 1), (v >> 29) & ((1 << 18) - 1), v >> 47           # offset, match length, literal length


def judged(c):
    """what the oracle says about a case as an archive entry: (zpack_result, bytes of the slot, produced, plain or None)"""
    o = oracle()
    cap = c["cap"] if c["cap"] is not None else max(1, c["uncomp"])
    rc, plain = o.zstd_decode(c["frame"], CAP)
    uncomp = len(plain) if rc == 0 and c["cap"] is None else c["uncomp"]
    h = o.xxh3(plain[:uncomp]) if rc == 0 else 0
    arc = zpk.assemble([c["frame"]], [("f", 10, len(c["frame"]), uncomp, h, 1)])
    erc, out, got, _ = o.entry_decode(arc, 10, len(c["frame"]), uncomp, h, 1, max(cap, uncomp) if c["cap"] is None else cap)
    return dict(rc=erc, out=out, produced=got, uncomp=uncomp, hash=h, cap=max(cap, uncomp) if c["cap"] is None else cap, arc=arc)


def test_the_table_holds_every_group_and_small_frames():
    groups = {}
    for c in Z.CASES:
        groups[c["group"]] = groups.get(c["group"], 0) + 1
        assert c["uncomp"] <= 256 << 10 and len(c["frame"]) <= 300 << 10, c["label"]
        assert c["two_stage"] in (True, None) or ":" in c["two_stage"], c["label"]          # declined by design: file:line
    assert sorted(groups) == list("ABCDEFGHI") and min(groups.values()) >= 6, groups


@pytest.mark.parametrize("group", list("ABCDEFGHI"))
def test_libzstd_and_the_oracle_agree_and_the_cases_sit_where_they_mean_to(libzstd, group):
    o = oracle()
    out = C.create_string_buffer(CAP)
    seen = 0
    for c in Z.CASES:
        if c["group"] != group:
            continue
        seen += 1
        e, label = c["expect"], c["label"]
        cap = c["cap"] if c["cap"] is not None else CAP
        r = libzstd.ZSTD_decompress(out, cap, c["frame"], len(c["frame"]))
        ok = not libzstd.ZSTD_isError(r)
        rc, seqs = o.zstd_sequences(c["frame"], cap, 1 << 16)
        bits = o.last_trace_bits
        st = o.zstd_stats()
        rc2, plain = o.zstd_decode(c["frame"], cap)
        assert rc == rc2 and ok == (rc == 0), (label, "libzstd valid", ok, "oracle", rc)
        if ok:
            assert out.raw[:r] == plain, (label, "bytes differ")
        if not e.get("libzstd_decides"):
            assert ok != bool(e.get("reject")), (label, "libzstd valid:", ok)
        j = judged(c)
        assert (j["rc"] == 0) == ok and (ok or j["rc"] in (12, 13)), (label, j["rc"])
        if have_ref():
            rr, reader, keep = ref().open_memory(j["arc"])
            assert rr == 0
            rrc, rout = ref().read_file(reader, 0, j["cap"])
            ref().close_reader(reader)
            assert rrc == j["rc"], (label, "reference", rrc, "oracle", j["rc"])
            if rrc == 0:
                assert rout[:j["uncomp"]] == j["out"][:j["uncomp"]], label
        if not ok:
            continue
        # ---- the label, from the oracle's statistics and trace ----
        if c["cap"] is None:
            assert len(plain) == c["uncomp"], (label, "the assembler's lengths", c["uncomp"], "decoded", len(plain))
        for k in STAT_FIELDS:
            if k in e:
                assert int(getattr(st, k)) == e[k], (label, k, int(getattr(st, k)), e[k])
        if "seq_modes" in e:
            assert e["seq_modes"] == c["modes"], label
            for kind in range(3):
                for mode in range(4):
                    assert st.seq_mode[kind][mode] == sum(1 for m in e["seq_modes"] if m[kind] == mode), (label, kind, mode)
        if "lit_fmt" in e:
            assert st.lit_huf_fmt[e["lit_fmt"]] == 1, (label, list(st.lit_huf_fmt))
        if "lit_small_fmt" in e:
            assert st.lit_small_fmt[e["lit_small_fmt"]] == 1 and sum(st.lit_small_fmt) == 1, (label, list(st.lit_small_fmt))
        if "ncount_on_byte" in e:
            assert st.ncount_on_byte == e["ncount_on_byte"], (label, st.ncount_on_byte)
        if "nseq_form" in e:
            assert st.nseq_form[e["nseq_form"]] >= 1, (label, list(st.nseq_form))
        if "fcs_bytes" in e:
            assert st.fcs_bytes == e["fcs_bytes"], (label, st.fcs_bytes)
        if "dict_id_bytes" in e:
            assert st.dict_id_bytes == e["dict_id_bytes"], (label, st.dict_id_bytes)
        if "block_regen_above_max" in e:
            assert st.block_max_regen > Z.BLOCK_MAX, (label, st.block_max_regen)
        t = [_unpack(v) for v in seqs]
        if "ll_values" in e:
            assert [x[2] for x in t] == e["ll_values"], (label, [x[2] for x in t])
        if "ml_values" in e:
            assert [x[1] for x in t] == e["ml_values"], (label, [x[1] for x in t])
        for i, off in e.get("offsets", {}).items():
            assert t[i][0] == off, (label, i, t[i], off)
        if "produced" in e:
            assert len(plain) == e["produced"], (label, len(plain))
        if "crosses" in e:               # a match that overlaps itself lies across this output position (of its block)
            pos, hit = e.get("block_at", 0), False
            for off, ml, ll in t:
                pos += ll
                hit |= off < ml and pos < e["crosses"] < pos + ml
                pos += ml
            assert hit, (label, e["crosses"])
        if "far_source" in e:            # a match whose source begins more than 4 KiB back and which runs for more than 1 KiB
            assert any(off > 4096 and ml > 1024 for off, ml, ll in t), label
        if e.get("all_orders"):          # the three history values, most recently used first, take all six orders
            hist, orders = [], set()
            for off, ml, ll in t:
                hist = [off] + [x for x in hist if x != off]
                if len(hist) >= 3:
                    orders.add(tuple(hist[:3]))
            vals = set(x for o3 in orders for x in o3)
            assert len(vals) == 3 and len(orders) == 6, (label, orders)
        if "big_seq" in e:
            k = t.index(e["big_seq"])
            before = int(bits[k - 1]) if k else None
            after = int(bits[k])
            where = e["big_seq_at"]
            if where == "top":
                assert k == 0, (label, k)
            elif where == "low":
                assert k == len(t) - 1, (label, k)
            else:                        # its bits lie across a 64-byte chunk boundary of the stream (zstd_fse4.h: chunk = bit position >> 9)
                assert before - after >= e["big_seq_bits"] - 26 and before - after > 64, (label, before, after)
                assert (before - 1) >> 9 != after >> 9 and after > 0, (label, before, after)
    assert seen >= 6
