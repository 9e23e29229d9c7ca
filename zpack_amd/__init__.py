"""zpack_amd — MI355X-native batch entry codec behind the ZPack C API.

The product is native: `libzpk_codec.so` (hand-written HIP kernels for gfx950 + the C-ABI of
include/zpack_codec.h) and `libzpack_amd.so` (the zpack.h reader/writer/stream API in C on top of it).
This package is a thin ctypes view for tests and bench.py.  There is no CPU fallback: if the HIP
library is missing or no device is usable, construction raises.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CODEC_SO = os.environ.get("ZPACK_AMD_CODEC_SO") or os.path.join(HERE, "libzpk_codec.so")     # override: A/B builds of the kernels
ZPACK_SO = os.path.join(HERE, "libzpack_amd.so")

METHOD_NONE, METHOD_ZSTD, METHOD_LZ4 = 0, 1, 2
DF_SKIP_HASH = 1
DF_GENERAL = 2
K_CLASSIFY, K_STORED, K_LZ4, K_ZSTD, K_ZSTD_FSE, K_PACK, K_ENCODE = 0, 1, 2, 3, 4, 5, 7
OPT_ENC_SPLIT_MIN, OPT_DEC_SPLIT_MIN, OPT_ORDER_MIN, OPT_ORDER_FAST_LAST = 6, 7, 8, 9      # zpk_codec_set_option (include/zpack_codec.h)
OPT_STORED_SPAN_MIN = 10
OPT_DIMAGE_CHUNK = 11
OPT_SPAN_HASH_MIN = 12
R_BASE_MISMATCH = 64                         # ZPK_R_BASE_MISMATCH: the per-entry status of a delta entry whose base did not hash to its value

# zpk_decode_desc / zpk_decode_result / zpk_encode_desc / zpk_encode_result (include/zpack_codec.h)
DECODE_DESC = np.dtype([("src_offset", "<u8"), ("comp_size", "<u8"), ("uncomp_size", "<u8"), ("expect_hash", "<u8"),
                        ("dst_offset", "<u8"), ("dst_capacity", "<u8"), ("method", "<u4"), ("flags", "<u4")])
DECODE_RESULT = np.dtype([("status", "<i4"), ("detail", "<u4"), ("produced", "<u8"), ("hash", "<u8")])
ENCODE_DESC = np.dtype([("src_offset", "<u8"), ("size", "<u8"), ("dst_offset", "<u8"), ("dst_capacity", "<u8"),
                        ("method", "<u4"), ("level", "<i4")])
ENCODE_RESULT = np.dtype([("status", "<i4"), ("detail", "<u4"), ("comp_size", "<u8"), ("hash", "<u8")])
assert DECODE_DESC.itemsize == 56 and DECODE_RESULT.itemsize == 24
assert ENCODE_DESC.itemsize == 40 and ENCODE_RESULT.itemsize == 24
PLANE_COPY = np.dtype([("src", "<u8"), ("dst", "<u8"), ("len", "<u8"), ("elem", "<u4"), ("join", "<u4")])       # zpk_plane_copy
assert PLANE_COPY.itemsize == 32
DELTA_COPY = np.dtype([("src", "<u8"), ("dst", "<u8"), ("base", "<u8"), ("len", "<u8"), ("elem", "<u4"), ("join", "<u4")])   # zpk_delta_copy
assert DELTA_COPY.itemsize == 40
HASH_SPAN = np.dtype([("addr", "<u8"), ("len", "<u8")])                                                         # zpk_hash_span
assert HASH_SPAN.itemsize == 16
WINDOW = np.dtype([("row_bytes", "<u8"), ("row0", "<u8"), ("rows", "<u8"), ("col0", "<u8"), ("cols", "<u8")])           # zpk_window (and zpack_amd_window)
WINDOW_COPY = np.dtype([("src", "<u8"), ("dst", "<u8"), ("base", "<u8"), ("n", "<u8"), ("win", WINDOW), ("elem", "<u4"), ("pad", "<u4")])   # zpk_window_copy
assert WINDOW.itemsize == 40 and WINDOW_COPY.itemsize == 80
PLACE_COPY = np.dtype([("src", "<u8"), ("dst", "<u8"), ("base", "<u8"), ("n", "<u8"), ("win", WINDOW), ("pitch", "<u8"), ("elem", "<u4"), ("pad", "<u4")])   # zpk_place_copy
assert PLACE_COPY.itemsize == 88


def slice_window(shape, dim, start, stop, itemsize=1):
    """The window (a WINDOW record's five values, in bytes) of the slice [start, stop) along dimension `dim` of a contiguous tensor of
    `shape` whose elements have `itemsize` bytes (include/zpack_codec.h states the formula).  ValueError: dim, start or stop out of range."""
    shape = [int(s) for s in shape]
    if not shape or any(s < 0 for s in shape):
        raise ValueError("shape %r" % (shape,))
    if not -len(shape) <= dim < len(shape):
        raise ValueError("dim %d of a %d-d shape" % (dim, len(shape)))
    dim %= len(shape)
    if not 0 <= start <= stop <= shape[dim]:
        raise ValueError("[%d, %d) of %d along dim %d" % (start, stop, shape[dim], dim))
    outer = inner = 1
    for s in shape[:dim]:
        outer *= s
    for s in shape[dim + 1:]:
        inner *= s
    inner *= int(itemsize)
    return (shape[dim] * inner, 0, outer, start * inner, (stop - start) * inner)


def place_of(dest_shape, dim, start, length, itemsize=1):
    """Where the slice [start, start + length) along dimension `dim` of a contiguous destination tensor of `dest_shape` lies, as
    (rows, cols, pitch, byte_offset), all but rows in bytes: the placement of a placed read (include/zpack_codec.h states the formula) —
    `rows` rows of `cols` bytes, row r at byte_offset + r * pitch of the tensor.  ValueError: dim, start or length out of range."""
    shape = [int(s) for s in dest_shape]
    if not shape or any(s < 0 for s in shape):
        raise ValueError("shape %r" % (shape,))
    if not -len(shape) <= dim < len(shape):
        raise ValueError("dim %d of a %d-d shape" % (dim, len(shape)))
    dim %= len(shape)
    if not (0 <= start and 0 <= length and start + length <= shape[dim]):
        raise ValueError("[%d, %d + %d) of %d along dim %d" % (start, start, length, shape[dim], dim))
    rows = inner = 1
    for s in shape[:dim]:
        rows *= s
    for s in shape[dim + 1:]:
        inner *= s
    inner *= int(itemsize)
    return (rows, length * inner, shape[dim] * inner, start * inner)


_lib = None


class CodecUnavailable(RuntimeError):
    pass


def lib():
    """Load libzpk_codec.so; raises (never falls back) when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(CODEC_SO):
            raise CodecUnavailable("%s is missing: run `python -m zpack_amd.build` (or __graft_entry__.build()); "
                                   "there is no CPU fallback" % CODEC_SO)
        # One HIP runtime per process: torch bundles its own libamdhip64.so.7; importing it first makes
        # the dynamic loader resolve this library's libamdhip64.so.7 dependency to the same copy.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(CODEC_SO)
        vp, u64, u8p = C.c_void_p, C.c_uint64, C.c_void_p
        L.zpk_codec_create.argtypes = [C.POINTER(vp), C.c_int]
        L.zpk_codec_destroy.argtypes = [vp]
        L.zpk_codec_destroy.restype = None
        L.zpk_codec_last_error.argtypes = [vp]
        L.zpk_codec_last_error.restype = C.c_char_p
        L.zpk_codec_device.argtypes = [vp]
        L.zpk_codec_decode_batch_device.argtypes = [vp, u8p, u64, vp, u64, u8p, u64, vp, vp]
        L.zpk_codec_decode_batch_host.argtypes = [vp, u8p, u64, vp, u64, vp, vp]
        L.zpk_codec_encode_batch_device.argtypes = [vp, u8p, u64, vp, u64, u8p, u64, vp, vp]
        L.zpk_codec_encode_batch_host.argtypes = [vp, vp, vp, u64, vp, vp]
        if hasattr(L, "zpk_codec_copy_spans_device"):         # (an A/B build from before the device-memory calls has none of them: using one raises)
            L.zpk_codec_decode_batch_host_dptr.argtypes = [vp, u8p, u64, vp, u64, vp, vp]
            L.zpk_codec_encode_batch_dsrc.argtypes = [vp, vp, vp, u64, vp, vp]
            L.zpk_codec_copy_spans_device.argtypes = [vp, vp, u64, vp]
            L.zpk_codec_pointer_device.argtypes = [vp]
            L.zpk_codec_packed_stride.argtypes = [u64]
            L.zpk_codec_packed_stride.restype = u64
        if hasattr(L, "zpk_codec_plane_copy_device"):         # (likewise: byte-plane entries)
            L.zpk_codec_plane_copy_device.argtypes = [vp, vp, u64, vp]
            L.zpk_codec_planes_stats.argtypes = [vp, C.POINTER(C.c_uint32)]
        if hasattr(L, "zpk_codec_delta_copy_device"):         # (likewise: delta entries)
            L.zpk_codec_delta_copy_device.argtypes = [vp, vp, u64, vp]
            L.zpk_codec_delta_stats.argtypes = [vp, C.POINTER(C.c_uint32)]
        if hasattr(L, "zpk_codec_hash_spans_device"):         # (likewise: spans hashed on the device, the base check)
            L.zpk_codec_hash_spans_device.argtypes = [vp, vp, u64, vp, vp]
            L.zpk_codec_base_check_stats.argtypes = [vp, C.POINTER(C.c_uint32)]
        if hasattr(L, "zpk_codec_window_copy_device"):        # (likewise: window reads)
            L.zpk_codec_window_copy_device.argtypes = [vp, vp, u64, vp]
            L.zpk_codec_window_stats.argtypes = [vp, C.POINTER(C.c_uint32)]
            L.zpk_codec_window_valid.argtypes = [u64, C.c_uint32, vp, C.POINTER(u64)]
            L.zpk_codec_window_overlap_ok.argtypes = [u64, u64, vp]
        if hasattr(L, "zpk_codec_place_copy_device"):         # (likewise: placed reads)
            L.zpk_codec_place_copy_device.argtypes = [vp, vp, u64, vp]
            L.zpk_codec_place_stats.argtypes = [vp, C.POINTER(C.c_uint32)]
            L.zpk_codec_place_valid.argtypes = [u64, C.c_uint32, vp, u64, C.POINTER(u64)]
            L.zpk_codec_place_overlap_ok.argtypes = [u64, u64, vp, u64]
        L.zpk_codec_pack_batch_device.argtypes = [vp, u8p, vp, vp, u64, u8p, u64, vp, u64, vp]
        L.zpk_codec_compress_bound.argtypes = [C.c_uint32, C.c_size_t]
        L.zpk_codec_compress_bound.restype = C.c_size_t
        L.zpk_codec_hash_batch_device.argtypes = [vp, u8p, vp, vp, u64, vp, vp]
        L.zpk_codec_hash_host.argtypes = [vp, u8p, u64, C.POINTER(u64)]
        L.zpk_codec_set_profiling.argtypes = [vp, C.c_int]
        L.zpk_codec_kernel_ms.argtypes = [vp, C.c_int, C.POINTER(C.c_float)]
        L.zpk_codec_debug_read.argtypes = [vp, vp, u64]
        L.zpk_codec_debug_fetch.argtypes = [vp, C.c_int, u64, vp, u64]
        L.zpk_codec_decode_stats.argtypes = [vp, C.POINTER(C.c_uint32)]
        L.zpk_codec_timer_start.argtypes = [vp, vp]
        L.zpk_codec_timer_stop.argtypes = [vp, vp, C.POINTER(C.c_float)]
        _lib = L
    return _lib


class Codec:
    """One codec context = one device (one process per GPU under torch.distributed)."""

    def __init__(self, device=-1):
        self.L = lib()
        h = C.c_void_p()
        rc = self.L.zpk_codec_create(C.byref(h), device)
        if rc != 0:
            raise CodecUnavailable("zpk_codec_create(device=%d) failed with %d: no usable HIP device; "
                                   "there is no CPU fallback" % (device, rc))
        self.h = h
        self.device = self.L.zpk_codec_device(h)

    def close(self):
        if getattr(self, "h", None):
            self.L.zpk_codec_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s failed (%d): %s" % (what, rc, self.L.zpk_codec_last_error(self.h).decode()))

    # ---- device-resident batch (torch uint8 CUDA tensors) ----
    # stream=None runs the batch on the codec's OWN stream, which is not ordered with torch's: fills / copies torch has enqueued on its
    # current stream for these tensors (a torch.zeros of the result array ...) must have finished before the codec touches them.
    @staticmethod
    def _settle(stream):
        if not stream:
            import sys
            t = sys.modules.get("torch")
            if t is not None and t.cuda.is_available() and t.cuda.is_initialized():
                t.cuda.current_stream().synchronize()

    def decode_batch_device(self, src, desc_dev, n, dst, results_dev, stream=None):
        self._settle(stream)
        st = C.c_void_p(stream) if stream else None
        self._chk(self.L.zpk_codec_decode_batch_device(self.h, src.data_ptr(), src.numel(), desc_dev.data_ptr(), n,
                                                       dst.data_ptr(), dst.numel(), results_dev.data_ptr(), st),
                  "zpk_codec_decode_batch_device")

    def decode_big_device(self, src, desc, dst):
        """ONE entry: src / dst are uint8 CUDA tensors, desc a one-element np array of DECODE_DESC (host) -> DECODE_RESULT (host, after the
        entry is decoded and verified)."""
        self._settle(None)
        desc = np.ascontiguousarray(desc, dtype=DECODE_DESC)
        res = np.zeros(1, dtype=DECODE_RESULT)
        self.L.zpk_codec_decode_big_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        self._chk(self.L.zpk_codec_decode_big_device(self.h, src.data_ptr(), src.numel(), desc.ctypes.data, dst.data_ptr(), dst.numel(), res.ctypes.data),
                  "zpk_codec_decode_big_device")
        return res[0]

    def decode_big_batch_device(self, src, desc, dst):
        """A batch that holds large entries: src / dst are uint8 CUDA tensors, desc an np array of DECODE_DESC (host) -> np array of
        DECODE_RESULT (host, after every entry is decoded and verified).  The block headers of the large LZ4 / Zstandard entries are walked
        on the device, so their compressed bytes stay there; the ones worth it are decoded block-parallel, large stored entries
        (OPT_STORED_SPAN_MIN) are copied and hashed chip-wide, the rest one wave each."""
        self._settle(None)
        desc = np.ascontiguousarray(desc, dtype=DECODE_DESC)
        res = np.zeros(len(desc), dtype=DECODE_RESULT)
        self.L.zpk_codec_decode_big_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
        self._chk(self.L.zpk_codec_decode_big_batch_device(self.h, src.data_ptr(), src.numel(), desc.ctypes.data, len(desc),
                                                           dst.data_ptr(), dst.numel(), res.ctypes.data),
                  "zpk_codec_decode_big_batch_device")
        return res

    def encode_batch_device(self, src, desc_dev, n, dst, results_dev, stream=None):
        self._settle(stream)
        st = C.c_void_p(stream) if stream else None
        self._chk(self.L.zpk_codec_encode_batch_device(self.h, src.data_ptr(), src.numel(), desc_dev.data_ptr(), n,
                                                       dst.data_ptr(), dst.numel(), results_dev.data_ptr(), st),
                  "zpk_codec_encode_batch_device")

    def encode_big_device(self, src, desc, dst, results_dev, stream=None):
        """A batch that holds large entries: src / dst / results_dev are uint8 CUDA tensors, desc an np array of ENCODE_DESC (host, consumed
        before the call returns).  Entries of at least OPT_ENC_SPLIT_MIN bytes are compressed in 512 KiB pieces and their frames assembled
        on the device; asynchronous like encode_batch_device."""
        self._settle(stream)
        st = C.c_void_p(stream) if stream else None
        desc = np.ascontiguousarray(desc, dtype=ENCODE_DESC)
        self.L.zpk_codec_encode_big_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        self._chk(self.L.zpk_codec_encode_big_device(self.h, src.data_ptr(), src.numel(), desc.ctypes.data, len(desc),
                                                     dst.data_ptr(), dst.numel(), results_dev.data_ptr(), st),
                  "zpk_codec_encode_big_device")

    def encode_stats(self):
        """The last encode_big_device call: entries written in pieces, and their pieces."""
        a = (C.c_uint32 * 8)()
        self.L.zpk_codec_encode_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        self._chk(self.L.zpk_codec_encode_stats(self.h, a), "encode_stats")
        return dict(split_entries=a[0], pieces=a[1])

    def pack_batch_device(self, slots, desc_dev, results_dev, n, packed, offsets_dev, max_entry_size, stream=None):
        """offsets_dev: int64 CUDA tensor of n + 1; packed: uint8 CUDA tensor or None (sizes only)."""
        self._settle(stream)
        st = C.c_void_p(stream) if stream else None
        self._chk(self.L.zpk_codec_pack_batch_device(self.h, slots.data_ptr(), desc_dev.data_ptr(), results_dev.data_ptr(), n,
                                                     packed.data_ptr() if packed is not None else None,
                                                     packed.numel() if packed is not None else 0, offsets_dev.data_ptr(),
                                                     max_entry_size, st), "zpk_codec_pack_batch_device")

    def hash_batch_device(self, src, offsets_dev, sizes_dev, n, hashes_dev, stream=None):
        self._settle(stream)
        st = C.c_void_p(stream) if stream else None
        self._chk(self.L.zpk_codec_hash_batch_device(self.h, src.data_ptr(), offsets_dev.data_ptr(), sizes_dev.data_ptr(),
                                                     n, hashes_dev.data_ptr(), st), "zpk_codec_hash_batch_device")

    def set_option(self, option, value):
        self.L.zpk_codec_set_option.argtypes = [C.c_void_p, C.c_int, C.c_int]
        self._chk(self.L.zpk_codec_set_option(self.h, option, value), "set_option")

    def set_profiling(self, on):
        self._chk(self.L.zpk_codec_set_profiling(self.h, 1 if on else 0), "set_profiling")

    def kernel_ms(self, which):
        ms = C.c_float(0)
        self._chk(self.L.zpk_codec_kernel_ms(self.h, which, C.byref(ms)), "kernel_ms")
        return ms.value

    def decode_stats(self):
        """Counters of the last decode batch: entries per method and how the Zstandard ones were finished."""
        a = (C.c_uint32 * 8)()
        self._chk(self.L.zpk_codec_decode_stats(self.h, a), "decode_stats")
        b = (C.c_uint32 * 16)()
        self.L.zpk_codec_decode_stats2.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        self._chk(self.L.zpk_codec_decode_stats2(self.h, b), "decode_stats2")
        return dict(stored=a[0], zstd=a[1], lz4=a[2], zstd_two_stage=a[3], zstd_fused=a[4], fse_watchdog=a[5], fse_budget=a[6],
                    zstd_arena_refused=bool(a[7] >> 31), retried_lz4=b[0], retried_zstd=b[1],
                    lz4_long_runs=b[3], lz4_handed_over=b[8], lz4_general=b[9],
                    frame_parallel_entries=b[5], frame_parallel_frames=b[6], zstd_blocks_flags=b[7],
                    device_walked=b[10], device_walk_accepted=b[11], stored_span_entries=b[12], stored_span_groups=b[13],
                    pipelined_sub_batches=b[14], span_copy_launches=b[15])

    def debug_fetch(self, what, offset, count, dtype):
        a = np.zeros(count, dtype=dtype)
        self._chk(self.L.zpk_codec_debug_fetch(self.h, what, offset, a.ctypes.data, a.nbytes), "debug_fetch")
        return a

    def debug_read(self, n):
        a = np.zeros((n, 8), dtype=np.uint64)
        self._chk(self.L.zpk_codec_debug_read(self.h, a.ctypes.data, a.nbytes), "debug_read")
        return a

    def timer_start(self, stream=None):
        self._chk(self.L.zpk_codec_timer_start(self.h, C.c_void_p(stream) if stream else None), "timer_start")

    def timer_stop(self, stream=None):
        ms = C.c_float(0)
        self._chk(self.L.zpk_codec_timer_stop(self.h, C.c_void_p(stream) if stream else None, C.byref(ms)), "timer_stop")
        return ms.value

    # ---- host-pointer forms (numpy) ----
    def decode_batch_host(self, archive, desc, caps=None):
        """archive: bytes/np.uint8; desc: np array of DECODE_DESC.  Returns (results, [output bytes])."""
        arc = np.ascontiguousarray(np.frombuffer(archive, dtype=np.uint8) if not isinstance(archive, np.ndarray) else archive)
        desc = np.ascontiguousarray(desc, dtype=DECODE_DESC)
        n = len(desc)
        outs = [np.zeros(max(1, int(d["dst_capacity"])), dtype=np.uint8) for d in desc]
        ptrs = (C.c_void_p * max(n, 1))(*[o.ctypes.data for o in outs])
        res = np.zeros(n, dtype=DECODE_RESULT)
        self._chk(self.L.zpk_codec_decode_batch_host(self.h, arc.ctypes.data, arc.size, desc.ctypes.data, n, ptrs,
                                                     res.ctypes.data), "zpk_codec_decode_batch_host")
        return res, [o[:int(d["dst_capacity"])] for o, d in zip(outs, desc)]

    # ---- the plaintext in the caller's DEVICE memory (torch tensors; archive and tables host memory) ----
    @staticmethod
    def _elem(elem, n):
        """the element sizes of a byte-plane call as the C array its last argument takes (None: NULL, the plain call)"""
        return None if elem is None else (C.c_uint8 * max(n, 1))(*[int(k) for k in elem])

    def decode_batch_host_dptr(self, archive, desc, dst_ptrs, elem=None):
        """decode_batch_host with device destinations: dst_ptrs[i] = device address of desc[i].dst_capacity bytes on this codec's device.
        elem: one element size per entry — those above 1 are byte-plane entries, joined on the way (None: the plain call).
        Returns the results; raises on ZPK_E_INVALID (a pointer the check turned down: nothing has run)."""
        self._settle(None)
        arc = np.ascontiguousarray(np.frombuffer(archive, dtype=np.uint8) if not isinstance(archive, np.ndarray) else archive)
        desc = np.ascontiguousarray(desc, dtype=DECODE_DESC)
        n = len(desc)
        ptrs = (C.c_void_p * max(n, 1))(*[int(p) if p else None for p in dst_ptrs])
        res = np.zeros(n, dtype=DECODE_RESULT)
        if elem is None:
            self._chk(self.L.zpk_codec_decode_batch_host_dptr(self.h, arc.ctypes.data, arc.size, desc.ctypes.data, n, ptrs, res.ctypes.data),
                      "zpk_codec_decode_batch_host_dptr")
            return res
        self.L.zpk_codec_decode_batch_host_dptr_planes.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        self._chk(self.L.zpk_codec_decode_batch_host_dptr_planes(self.h, arc.ctypes.data, arc.size, desc.ctypes.data, n, ptrs, res.ctypes.data, self._elem(elem, n)),
                  "zpk_codec_decode_batch_host_dptr_planes")
        return res

    # ---- the ARCHIVE IMAGE in the caller's device memory (a uint8 CUDA tensor; the tables host memory) ----
    def decode_batch_dimage(self, image, desc, dst_ptrs=None, elem=None):
        """decode_batch_host / decode_batch_host_dptr with the archive in device memory.  dst_ptrs None: host destinations — returns
        (results, [output bytes]) like decode_batch_host; else dst_ptrs[i] = device address of desc[i].dst_capacity bytes on this codec's
        device — returns the results; elem: as in decode_batch_host_dptr.  Raises on ZPK_E_INVALID (a pointer the check turned down:
        nothing has run)."""
        self._settle(None)
        desc = np.ascontiguousarray(desc, dtype=DECODE_DESC)
        n = len(desc)
        res = np.zeros(n, dtype=DECODE_RESULT)
        self.L.zpk_codec_decode_batch_dimage.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_void_p]
        if dst_ptrs is None:
            outs = [np.zeros(max(1, int(d["dst_capacity"])), dtype=np.uint8) for d in desc]
            ptrs = (C.c_void_p * max(n, 1))(*[o.ctypes.data for o in outs])
        else:
            ptrs = (C.c_void_p * max(n, 1))(*[int(p) if p else None for p in dst_ptrs])
        if elem is None:
            self._chk(self.L.zpk_codec_decode_batch_dimage(self.h, image.data_ptr(), image.numel(), desc.ctypes.data, n, ptrs,
                                                           0 if dst_ptrs is None else 1, res.ctypes.data), "zpk_codec_decode_batch_dimage")
        else:
            self.L.zpk_codec_decode_batch_dimage_planes.argtypes = self.L.zpk_codec_decode_batch_dimage.argtypes + [C.c_void_p]
            self._chk(self.L.zpk_codec_decode_batch_dimage_planes(self.h, image.data_ptr(), image.numel(), desc.ctypes.data, n, ptrs,
                                                                  0 if dst_ptrs is None else 1, res.ctypes.data, self._elem(elem, n)),
                      "zpk_codec_decode_batch_dimage_planes")
        if dst_ptrs is None:
            return res, [o[:int(d["dst_capacity"])] for o, d in zip(outs, desc)]
        return res

    def dimage_stats(self):
        """The last decode_batch_dimage call: its sub-batches (OPT_DIMAGE_CHUNK), k_span_copy launches and the bytes it copied home."""
        a = (C.c_uint32 * 4)()
        self.L.zpk_codec_dimage_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        self._chk(self.L.zpk_codec_dimage_stats(self.h, a), "zpk_codec_dimage_stats")
        return dict(sub_batches=a[0], span_copy_launches=a[1], bytes_copied_home=a[2])

    # ---- a batch that is only TESTED: the verdicts of decode_batch_host / decode_batch_dimage, no plaintext anywhere ----
    def verify_batch_host(self, archive, desc):
        """archive: bytes/np.uint8 (host); desc: np array of DECODE_DESC, dst_offset / dst_capacity ignored.  Returns the results."""
        arc = np.ascontiguousarray(np.frombuffer(archive, dtype=np.uint8) if not isinstance(archive, np.ndarray) else archive)
        desc = np.ascontiguousarray(desc, dtype=DECODE_DESC)
        res = np.zeros(len(desc), dtype=DECODE_RESULT)
        self.L.zpk_codec_verify_batch_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
        self._chk(self.L.zpk_codec_verify_batch_host(self.h, arc.ctypes.data, arc.size, desc.ctypes.data, len(desc), res.ctypes.data),
                  "zpk_codec_verify_batch_host")
        return res

    def verify_batch_dimage(self, image, desc):
        """... with the archive image in device memory (a uint8 CUDA tensor on this codec's device)."""
        self._settle(None)
        desc = np.ascontiguousarray(desc, dtype=DECODE_DESC)
        res = np.zeros(len(desc), dtype=DECODE_RESULT)
        self.L.zpk_codec_verify_batch_dimage.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
        self._chk(self.L.zpk_codec_verify_batch_dimage(self.h, image.data_ptr(), image.numel(), desc.ctypes.data, len(desc), res.ctypes.data),
                  "zpk_codec_verify_batch_dimage")
        return res

    def verify_stats(self):
        """The last verify_batch_* call: its sub-batches (OPT_DIMAGE_CHUNK), the stored entries hashed in place and the plaintext bytes
        that came home (0)."""
        a = (C.c_uint32 * 4)()
        self.L.zpk_codec_verify_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        self._chk(self.L.zpk_codec_verify_stats(self.h, a), "zpk_codec_verify_stats")
        return dict(sub_batches=a[0], stored_hashed_in_place=a[1], bytes_copied_home=a[2])

    # ---- a bounded SINK in the caller's device memory (a uint8 CUDA tensor; sources host arrays or device addresses; the tables host memory) ----
    def encode_batch_dsink(self, srcs, desc, sink, sink_offset=0, room=None, src_on_device=False, elem=None):
        """encode_batch_host / _dsrc whose payloads are committed back to back to sink[sink_offset, sink_offset + room) under the append
        rule (zpack_codec.h): srcs[i] is a np.uint8 array (host) or a device address (src_on_device) of desc[i].size bytes.  Returns
        (results, placed, bytes).  elem (device sources): one element size per entry — those above 1 are split into byte planes on the
        way into the staging (None: the plain call).  Raises on ZPK_E_INVALID (a pointer the check turned down: nothing has run)."""
        self._settle(None)
        desc = np.ascontiguousarray(desc, dtype=ENCODE_DESC)
        n = len(desc)
        if src_on_device:
            ptrs = (C.c_void_p * max(n, 1))(*[int(p) if p else None for p in srcs])
        else:
            keep = [np.ascontiguousarray(a, dtype=np.uint8) for a in srcs]
            ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data if a.size else None for a in keep])
        if room is None:
            room = sink.numel() - sink_offset
        res = np.zeros(n, dtype=ENCODE_RESULT)
        placed, nbytes = C.c_uint64(0), C.c_uint64(0)
        self.L.zpk_codec_encode_batch_dsink.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p,
                                                        C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        if elem is None:
            self._chk(self.L.zpk_codec_encode_batch_dsink(self.h, ptrs, 1 if src_on_device else 0, desc.ctypes.data, n, sink.data_ptr() + sink_offset, room,
                                                          res.ctypes.data, C.byref(placed), C.byref(nbytes)), "zpk_codec_encode_batch_dsink")
        else:
            self.L.zpk_codec_encode_batch_dsink_planes.argtypes = self.L.zpk_codec_encode_batch_dsink.argtypes + [C.c_void_p]
            self._chk(self.L.zpk_codec_encode_batch_dsink_planes(self.h, ptrs, 1 if src_on_device else 0, desc.ctypes.data, n, sink.data_ptr() + sink_offset, room,
                                                                 res.ctypes.data, C.byref(placed), C.byref(nbytes), self._elem(elem, n)),
                      "zpk_codec_encode_batch_dsink_planes")
        return res, placed.value, nbytes.value

    def dsink_stats(self):
        """The last encode_batch_dsink call: its sub-batches (OPT_DIMAGE_CHUNK) and the workgroups of its last k_sink_place launch."""
        a = (C.c_uint32 * 4)()
        self.L.zpk_codec_dsink_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        self._chk(self.L.zpk_codec_dsink_stats(self.h, a), "zpk_codec_dsink_stats")
        return dict(sub_batches=a[0], place_groups=a[1])

    def copy_spans_device(self, rows, stream=None):
        """rows: (n, 3) uint64 array of (src address, dst address, len): one k_span_copy launch, asynchronous on `stream` (None: the
        codec's own; synchronise the device before reading the destinations)."""
        self._settle(stream)
        rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, 3)
        self._chk(self.L.zpk_codec_copy_spans_device(self.h, rows.ctypes.data, len(rows), C.c_void_p(stream) if stream else None),
                  "zpk_codec_copy_spans_device")

    def plane_copy_device(self, rows, stream=None):
        """rows: PLANE_COPY array of (src address, dst address, len, elem, join): one k_plane_copy launch — join 0 groups the bytes of
        elements of `elem` bytes into planes (include/zpack_codec.h states the layout), join 1 puts them back —, asynchronous on `stream`
        (None: the codec's own; synchronise the device before reading the destinations)."""
        self._settle(stream)
        rows = np.ascontiguousarray(rows, dtype=PLANE_COPY)
        self._chk(self.L.zpk_codec_plane_copy_device(self.h, rows.ctypes.data, len(rows), C.c_void_p(stream) if stream else None),
                  "zpk_codec_plane_copy_device")

    def delta_copy_device(self, rows, stream=None):
        """rows: DELTA_COPY array of (src address, dst address, base address, len, elem, join): one k_delta_copy launch — join 0 takes plain
        bytes to split(plain ^ base), join 1 stored bytes to join(stored) ^ base (include/zpack_codec.h states the layout); on a join
        base == dst is legal.  Asynchronous on `stream` (None: the codec's own; synchronise the device before reading the destinations).
        Raises on ZPK_E_INVALID (a pointer, a missing base or an overlap the check turned down: nothing has run)."""
        self._settle(stream)
        rows = np.ascontiguousarray(rows, dtype=DELTA_COPY)
        self._chk(self.L.zpk_codec_delta_copy_device(self.h, rows.ctypes.data, len(rows), C.c_void_p(stream) if stream else None),
                  "zpk_codec_delta_copy_device")

    def delta_stats(self):
        """The most recent call that could split or join: rows split with a base, rows joined with a base, k_delta_copy launches, entries
        that decoded into the staging only because they had a base."""
        a = (C.c_uint32 * 4)()
        self._chk(self.L.zpk_codec_delta_stats(self.h, a), "zpk_codec_delta_stats")
        return dict(split=a[0], joined=a[1], launches=a[2], staged=a[3])

    def window_copy_device(self, rows, stream=None):
        """rows: WINDOW_COPY array of (src address, dst address, base address or 0, n, window, elem): one k_window_copy launch — the window
        of the n stored bytes at src, joined and XORed with the base, densely to dst (include/zpack_codec.h states the map); base == dst
        is legal.  Asynchronous on `stream` (None: the codec's own; synchronise the device before reading the destinations).  Raises on
        ZPK_E_INVALID (a window, a pointer or an overlap the check turned down: nothing has run)."""
        self._settle(stream)
        rows = np.ascontiguousarray(rows, dtype=WINDOW_COPY)
        self._chk(self.L.zpk_codec_window_copy_device(self.h, rows.ctypes.data, len(rows), C.c_void_p(stream) if stream else None),
                  "zpk_codec_window_copy_device")

    def window_stats(self):
        """The most recent call that could split, join or cut a window: rows windowed, k_window_copy launches, entries that decoded into
        the staging only because they had a window."""
        a = (C.c_uint32 * 3)()
        self._chk(self.L.zpk_codec_window_stats(self.h, a), "zpk_codec_window_stats")
        return dict(rows=a[0], launches=a[1], staged=a[2])

    def place_copy_device(self, rows, stream=None):
        """rows: PLACE_COPY array of (src address, dst address, base address or 0, n, window, pitch, elem): one k_place_copy launch — the
        window of the n stored bytes at src, joined and XORed with the base, window row r at r * pitch of dst (include/zpack_codec.h
        states the map); the gaps between the rows are not touched, so several rows may share one destination tensor; base == dst is
        legal.  Asynchronous on `stream` (None: the codec's own; synchronise the device before reading the destinations).  Raises on
        ZPK_E_INVALID (a placement, a pointer or an overlap the check turned down: nothing has run)."""
        self._settle(stream)
        rows = np.ascontiguousarray(rows, dtype=PLACE_COPY)
        self._chk(self.L.zpk_codec_place_copy_device(self.h, rows.ctypes.data, len(rows), C.c_void_p(stream) if stream else None),
                  "zpk_codec_place_copy_device")

    def place_stats(self):
        """The most recent call that could split, join, cut or place: rows placed, k_place_copy launches."""
        a = (C.c_uint32 * 2)()
        self._chk(self.L.zpk_codec_place_stats(self.h, a), "zpk_codec_place_stats")
        return dict(rows=a[0], launches=a[1])

    def hash_spans_device(self, rows, stream=None):
        """rows: HASH_SPAN array of (device address, len), any alignment: the XXH3-64 (seed 0) of each span as a uint64 array — rows below
        OPT_SPAN_HASH_MIN one wave each in one k_span_hash launch, the others chip-wide.  Synchronous: the hashes are home on return.
        Raises on ZPK_E_INVALID (a span the pointer check turned down: nothing has run)."""
        self._settle(stream)
        rows = np.ascontiguousarray(rows, dtype=HASH_SPAN)
        out = np.zeros(len(rows), dtype=np.uint64)
        self._chk(self.L.zpk_codec_hash_spans_device(self.h, rows.ctypes.data, len(rows), out.ctypes.data, C.c_void_p(stream) if stream else None),
                  "zpk_codec_hash_spans_device")
        return out

    def base_check_stats(self):
        """The most recent call that hashed spans (hash_spans_device, a _delta_checked read): spans hashed by one wave, spans hashed
        chip-wide, bases that did not hash to their value, kernel launches of the pass."""
        a = (C.c_uint32 * 4)()
        self._chk(self.L.zpk_codec_base_check_stats(self.h, a), "zpk_codec_base_check_stats")
        return dict(wave=a[0], wide=a[1], refused=a[2], launches=a[3])

    def planes_stats(self):
        """The most recent call that could split or join byte planes: rows split, rows joined, k_plane_copy launches, entries that decoded
        into the staging only because they were grouped."""
        a = (C.c_uint32 * 4)()
        self._chk(self.L.zpk_codec_planes_stats(self.h, a), "zpk_codec_planes_stats")
        return dict(split=a[0], joined=a[1], launches=a[2], staged=a[3])

    def hash_host(self, data):
        a = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8))
        h = C.c_uint64(0)
        self._chk(self.L.zpk_codec_hash_host(self.h, a.ctypes.data if a.size else None, a.size, C.byref(h)), "zpk_codec_hash_host")
        return h.value

    def compress_bound(self, method, n):
        return self.L.zpk_codec_compress_bound(method, n)


def decode_descs_from_batch(batch, dst_align=256, flags=0):
    """Descriptors for every entry of a benchdata Batch (or any object with the same arrays), output
    slots laid out back to back (aligned); returns (desc, total_dst_bytes)."""
    n = batch.n
    d = np.zeros(n, dtype=DECODE_DESC)
    d["src_offset"] = batch.offsets
    d["comp_size"] = batch.comp_sizes
    d["uncomp_size"] = batch.uncomp_sizes
    d["expect_hash"] = batch.hashes
    d["dst_capacity"] = batch.uncomp_sizes
    d["method"] = batch.methods
    d["flags"] = flags
    sizes = (batch.uncomp_sizes.astype(np.uint64) + np.uint64(dst_align - 1)) & ~np.uint64(dst_align - 1)
    offs = np.zeros(n, dtype=np.uint64)
    if n > 1:
        offs[1:] = np.cumsum(sizes[:-1])
    d["dst_offset"] = offs
    total = int(offs[-1] + sizes[-1]) if n else 0
    return d, total
