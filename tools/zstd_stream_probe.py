"""Stream-decode the Zstandard fixtures of tests/golden/foreign_frames.json (zstd:skippable_between_frames first, alone, then all in file
order) with the codec library named by ZPACK_AMD_CODEC_SO, each against the one-shot decode of the same bytes.  After a stream that ends
with another verdict, print zpk_stream_rec (rc, fired, produced) and the head of ZstdResume, read back on the host: the kernels are
not touched (profiles/r11/README.md).  The record's address is taken from zpk_dstream::d_aux (zpk_stream.inc), offset 56 on x86-64."""
import ctypes as C, json, os, struct, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
torch.zeros(1, device="cuda:0")
import zpack_amd
from benchdata import datagen as dg
from tests import zpk
from tests.test_gpu_codec import _desc

def hip():
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no hip runtime loaded")

def dump(H, s):
    d_aux = C.c_uint64.from_address(s.value + 56).value
    if not d_aux:
        return "no aux"
    buf = (C.c_uint8 * 384)()
    H.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    rc = H.hipMemcpy(buf, d_aux, 384, 2)
    b = bytes(buf)
    rcv, fired, produced, hsh = struct.unpack_from("<iIQQ", b, 0)
    ip_off, op_off, flo, fcs, pad = struct.unpack_from("<5Q", b, 256)
    rep = struct.unpack_from("<3Q", b, 256 + 40)
    phase, fn, ck, stv = struct.unpack_from("<4I", b, 256 + 64)
    al = struct.unpack_from("<4i", b, 256 + 80)
    return "memcpy=%d rec{rc=%d fired=%u produced=%u} zr{ip_off=%u op_off=%u frame_lo=%u fcs=%u pad=%u rep=%s phase=%u fn=%u cksum=%u stv=%u al=%s}" % (
        rc, rcv, fired, produced, ip_off, op_off, flo, fcs, pad, rep, phase, fn, ck, stv, al)

def stream(codec, H, frame, method, usize, h, chunk, out_chunk=4096):
    L = codec.L
    L.zpk_dstream_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.zpk_dstream_destroy.argtypes = [C.c_void_p]; L.zpk_dstream_destroy.restype = None
    L.zpk_dstream_step.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                   C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    L.zpk_dstream_wants_input.argtypes = [C.c_void_p]
    L.zpk_dstream_counters.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    s = C.c_void_p()
    assert L.zpk_dstream_create(codec.h, C.byref(s)) == 0
    src = np.frombuffer(frame, dtype=np.uint8)
    ob = np.zeros(out_chunk, dtype=np.uint8)
    out = bytearray(); pos = 0; status = 0
    consumed, produced, done = C.c_size_t(0), C.c_size_t(0), C.c_int(0)
    for _ in range(1000000):
        take = min(chunk, len(src) - pos) if L.zpk_dstream_wants_input(s) else 0
        rc = L.zpk_dstream_step(s, method, len(src), usize, h, src[pos:].ctypes.data if take else None, take, C.byref(consumed),
                                ob.ctypes.data, out_chunk, C.byref(produced), C.byref(done))
        assert rc != 1001
        pos += consumed.value
        out += ob[:produced.value].tobytes()
        status = rc
        if rc != 0 or done.value:
            break
        assert consumed.value or produced.value
    la, ca = C.c_uint64(0), C.c_uint64(0)
    L.zpk_dstream_counters(s, C.byref(la), C.byref(ca))
    d = dump(H, s)
    L.zpk_dstream_destroy(s)
    return status, bytes(out), la.value, d

def main():
    print("codec:", zpack_amd.CODEC_SO, flush=True)
    codec = zpack_amd.Codec(0)
    H = hip()
    cases = [c for c in json.load(open(os.path.join(ROOT, "tests", "golden", "foreign_frames.json")))
             if c["max_size"] == c["uncomp_size"] and c["uncomp_size"] > 0 and c["label"].startswith("zstd:")]
    def run(c, chunk, tag):
        fr = bytes.fromhex(c["frame"]); usize = c["uncomp_size"]; h = c["hash"]
        e = dict(offset=10, comp_size=len(fr), uncomp_size=usize, hash=h, method=c["method"])
        arc = zpk.assemble([fr], [("f", 10, len(fr), usize, h, c["method"])])
        res, outs = codec.decode_batch_host(arc, _desc([e], [usize]))
        want = int(res[0]["status"]); prod = int(res[0]["produced"])
        if want == 0 and prod < usize: want = 15
        st, got, launches, d = stream(codec, H, fr, c["method"], usize, h, chunk)
        same = st == want and (want not in (0, 15) or got == outs[0][:min(prod, usize)].tobytes())
        print("%s %-40s chunk %5d one-shot %2d stream %2d launches %d %s%s" % (tag, c["label"], chunk, want, st, launches, "OK" if same else "MISMATCH", "" if same else " " + d), flush=True)
        return same
    bad = 0
    first = [c for c in cases if c["label"] == "zstd:skippable_between_frames"][0]
    bad += not run(first, 1000, "alone-first")
    bad += not run(first, 1000, "alone-again")
    for c in cases:
        bad += not run(c, 1000, "in-order   ")
    print("mismatches:", bad, flush=True)

main()
