"""GPU: the four row tables of one codec in ONE read call, and again (zpack_amd/csrc/zpk_codec.hip: row_table_enqueue behind rows_enqueue).

A call whose batch holds plain, byte-plane, delta and windowed entries fills the tables of k_span_copy, k_plane_copy, k_delta_copy and
k_window_copy before any of the kernels has run; the same call a second time writes each table's pinned block again, behind the event of
its own last upload.  The archive is built on the host with numpy — stored = split_k(plain XOR base) —, so every destination has a model
that no code of the codec made."""
import ctypes as C

import numpy as np
import pytest

import zpack_amd
from benchdata import datagen as dg
from tests import zpk
from tests.device_mem import torch, _layout, _build, CANARY            # noqa: F401  (torch: fixture)

pytestmark = pytest.mark.gpu

PIECE = 16384                                                           # one work item of every table (copy_rows_plan.h)
MIS = (0, 1, 7, 15)


def _size(k):
    """a row of two items: one whole piece, then one wide group of 16 elements and one loose element"""
    return PIECE + 16 * k + k


def _split(plain, k):
    m = plain.size // k
    return np.concatenate([plain[:m * k].reshape(m, k).T.reshape(-1), plain[m * k:]])


# the windowed entries: a matrix of 9 rows x 1844 bytes (n = 16596: _size(4) = 16452 rounded up to whole rows), of which the window takes
# the bytes [8, 1836) of every row: 9 x 1828 = 16452 = _size(4) destination bytes.  Byte 16384 of the destination lies 1760 bytes into
# window row 8, so the second item is the last 68 bytes of that row: one group of 64 and 4 loose bytes.
ROW_BYTES, NROWS, ROW0, ROWS, COL0, COLS = 1844, 9, 0, 9, 8, 1828
WINDOW = (ROW_BYTES, ROW0, ROWS, COL0, COLS)
WHOLE = (0, 0, 0, 0, 0)


def _cut(raw):
    return np.ascontiguousarray(raw.reshape(NROWS, ROW_BYTES)[ROW0:ROW0 + ROWS, COL0:COL0 + COLS]).reshape(-1)


@pytest.fixture(scope="module")
def batch():
    """six entries: plain uint8 | byte planes, k = 4 | delta, k = 2 | window, k = 4 | window with a base, k = 4 | no bytes"""
    assert ROWS * COLS == _size(4) and NROWS * ROW_BYTES == -(-_size(4) // ROW_BYTES) * ROW_BYTES
    rng = np.random.default_rng(36)
    n = [_size(1), _size(4), _size(2), NROWS * ROW_BYTES, NROWS * ROW_BYTES, 0]
    elem = [1, 4, 2, 4, 4, 1]
    plain = [rng.integers(0, 256, s, dtype=np.uint8) for s in n]
    base = [None, None, rng.integers(0, 256, n[2], dtype=np.uint8), None, rng.integers(0, 256, n[4], dtype=np.uint8), None]
    stored = [_split(p if b is None else p ^ b, k) for p, b, k in zip(plain, base, elem)]
    image = _build([(dg.LZ4, 0, s.tobytes()) for s in stored])
    wins = [WHOLE, WHOLE, WHOLE, WINDOW, WINDOW, WHOLE]
    want = [_cut(p) if w is not WHOLE else p for p, w in zip(plain, wins)]
    given = [b if b is None or w is WHOLE else _cut(b) for b, w in zip(base, wins)]     # the base of a window is its shard
    assert [w.size for w in want] == [_size(1), _size(4), _size(2), _size(4), _size(4), 0]
    return dict(image=image, elem=elem, wins=wins, want=want, base=given)


def test_one_call_fills_all_four_tables_and_a_second_call_waits_for_each(torch, batch):
    L = zpack_amd.lib()
    vp, u64 = C.c_void_p, C.c_uint64
    L.zpk_codec_decode_batch_host_dptr_windows.argtypes = [vp, vp, u64, vp, u64, vp, vp, vp, vp, vp, vp]
    ents = zpk.parse(batch["image"])
    want, n = batch["want"], len(ents)
    caps = [w.size for w in want]
    dd = np.zeros(n, dtype=zpack_amd.DECODE_DESC)
    for i, e in enumerate(ents):
        dd[i] = (e["offset"], e["comp_size"], e["uncomp_size"], e["hash"], 0, caps[i], e["method"], 0)
    arc = np.frombuffer(batch["image"], dtype=np.uint8)
    boffs, btotal = _layout([0 if b is None else b.size for b in batch["base"]], (7, 0, 15, 1))
    bh = np.full(btotal, CANARY, dtype=np.uint8)
    for b, x in zip(batch["base"], boffs):
        if b is not None:
            bh[x:x + b.size] = b
    bbuf = torch.from_numpy(bh).to("cuda:0")
    c_base = (C.c_void_p * n)(*[None if b is None else bbuf.data_ptr() + x for b, x in zip(batch["base"], boffs)])
    c_elem = (C.c_uint8 * n)(*batch["elem"])
    wins = np.array(batch["wins"], dtype=zpack_amd.WINDOW)
    codec = zpack_amd.Codec(0)
    try:
        for turn, mis in enumerate((MIS, MIS[::-1])):                                   # fresh destinations each time, at other alignments
            offs, total = _layout(caps, mis)
            model = np.full(total, CANARY, dtype=np.uint8)
            for x, w in zip(offs, want):
                model[x:x + w.size] = w
            out = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda:0")
            c_dst = (C.c_void_p * n)(*[out.data_ptr() + x for x in offs])
            res = np.zeros(n, dtype=zpack_amd.DECODE_RESULT)
            torch.cuda.synchronize()
            rc = L.zpk_codec_decode_batch_host_dptr_windows(codec.h, arc.ctypes.data, arc.size, dd.ctypes.data, n, c_dst, res.ctypes.data, c_elem, c_base, None, wins.ctypes.data)
            torch.cuda.synchronize()
            ps, ds, ws, spans = codec.planes_stats(), codec.delta_stats(), codec.window_stats(), codec.decode_stats()["span_copy_launches"]
            print("turn %d: rc %d status %s planes %s delta %s window %s span copy launches %d" % (turn, rc, list(res["status"]), ps, ds, ws, spans))
            assert rc == 0 and (res["status"] == 0).all(), (turn, rc, list(res["status"]))
            got = out.cpu().numpy()
            bad = np.flatnonzero(got != model)
            assert bad.size == 0, (turn, int(bad[0]), bad.size, offs)                   # every destination and every guard byte around it
            assert np.array_equal(bbuf.cpu().numpy(), bh)                               # the bases are only read
            assert ps["joined"] == 1 and ps["launches"] == 1, (turn, ps)
            assert ds["joined"] == 1 and ds["launches"] == 1, (turn, ds)
            assert ws["rows"] == 2 and ws["launches"] == 1, (turn, ws)
            assert spans == 1, (turn, spans)                                            # the plain entry; the entry of no bytes takes no row
    finally:
        codec.close()
