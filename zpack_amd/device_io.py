"""Archives read into and written from CUDA tensors: the plaintext stays in device memory, only compressed bytes cross the bus.

A thin ctypes view of the three device-memory calls of libzpack_amd.so (include/zpack_amd.h: zpack_amd_read_files_device,
zpack_amd_read_files_device_packed, zpack_amd_write_files_device), of the verdict-only read (zpack_amd_test_files), of the reader over an archive image in device memory
(zpack_amd_init_reader_device) and of the writer whose sink is one (zpack_amd_init_writer_device), with torch for the memory.  There is no CPU fallback: without a HIP device the calls return
ZPACK_ERROR_NOT_AVAILABLE and these functions raise.

    tensors, statuses = read_files_device("weights.zpk")                  # every entry, in archive order
    tensors, statuses = read_files_device(image)                          # ... of an archive that lies in a uint8 CUDA tensor
    write_files_device("weights.zpk", {"layer0": t0, "layer1": t1}, method=METHOD_LZ4, level=0)
    image = write_archive_device({"layer0": t0, "layer1": t1})            # the archive as a uint8 CUDA tensor: no compressed byte crosses the bus
    statuses = test_files(image)                                          # every entry decoded and hashed on the device: verdicts, no tensor
    image = write_archive_device({"layer0": t0, ...}, planes="dtype")      # float tensors stored as byte planes: they compress (below)
    tensors, statuses = read_files_device(image, planes="manifest")       # ... and come back as they were

Byte planes (include/zpack_amd.h: zpack_amd_write_files_device_planes, zpack_amd_read_files_device_planes).  A float tensor alternates
bytes that compress with bytes that are noise; an entry with element size k in {2, 4, 8} is stored with byte 0 of every element first,
then byte 1 of every element, and so on.  The grouping happens inside the copy the codec makes of the plaintext anyway.  `planes` is
{name: element size} (names left out: 1) or, writing, "dtype": tensor.element_size() for floating dtypes of 2, 4 or 8 bytes, 1 for
everything else — the writer then appends one stored entry, PLANES_MANIFEST, that holds the map as JSON, and read_files_device(...,
planes="manifest") applies it.  To any other reader a grouped entry is an ordinary entry whose bytes are the grouped bytes.

Delta entries (include/zpack_amd.h: zpack_amd_write_files_device_delta, zpack_amd_read_files_device_delta).  What compresses in a
checkpoint is its difference to the previous one: with base={name: tensor} — the previous checkpoint's tensors, which lie in device
memory anyway — an entry is stored as the byte planes of `tensor XOR base`, and read_files_device(..., base=...) hands back the tensor.
inplace=True reads into the base tensors themselves: the previous checkpoint becomes the new one, without a second copy.  The base is
not in the archive; with planes="dtype" the writer appends DELTA_MANIFEST, the names of the delta entries and the caller's `base_id`,
and planes="manifest" refuses to hand out a delta entry for which no base was given.

The base is checked before it is applied (zpack_amd_hash_device, zpack_amd_read_files_device_delta_checked).  An entry's hash is over its
stored bytes, so a read against the wrong base would decode, verify and return garbage — in place, over the only copy of the previous
checkpoint.  With check_base=True the writers hash the bases on the device and record "base_xxh3": {name: 16 hex digits} in
DELTA_MANIFEST beside the two fields it has (without it the manifest is written as it always was), and read_files_device(...,
planes="manifest", base=...) of such an archive hashes the bases it is given on the device first: an entry whose base differs comes
back with status BASE_MISMATCH and its tensor — with inplace=True the base itself — untouched.  `base_id` stays what it was, a string
of the caller's; check_base=False on the read is the read without the check.

    image = write_archive_device(new, planes="dtype", base=old, base_id="step 1000", check_base=True)  hash_tensors(tensors) gives the same values on their own:
the `hash` field an archive records for an entry with those bytes.

    image = write_archive_device(new, planes="dtype", base=old, base_id="step 1000")
    tensors, statuses = read_files_device(image, planes="manifest", base=old, base_id="step 1000", inplace=True)     # `old` now holds `new`

Window reads (include/zpack_amd.h: zpack_amd_read_files_device_windows).  A checkpoint loaded under another layout than it was written
under — tensor-parallel ranks, a pipeline stage — needs a slice of every tensor.  With window={name: (shape, dim, start, stop)} the
tensor returned for an entry holds the slice [start, stop) along `dim` of the entry seen as a contiguous tensor of `shape`, cut inside
the copy that delivers the entry: no full-size tensor is allocated and no second pass runs.  With base= the base is the caller's shard
of the previous checkpoint, of the slice's size, and inplace=True reads into it.

    mine, statuses = read_files_device(image, planes="manifest", window={"w": ((4096, 4096), 1, 0, 512)})    # columns [0, 512) of w

Placed reads (include/zpack_amd.h: zpack_amd_read_files_device_placed).  The opposite direction: a checkpoint written by several
tensor-parallel ranks holds one shard entry per rank and weight, and a loader at another width puts shards side by side in one tensor.
With place={name: (dest_tensor, dim, start)} the entry — or its `window` slice — lands at [start, start + length) along `dim` of the
caller's contiguous `dest_tensor`, placed inside the copy that delivers the entry: no scratch tensor per shard and no torch.cat.  The
tensor returned for such an entry is `dest_tensor`.  Four column shards of a (4096, 4096) bf16 weight merged by one read:

    w = torch.empty(4096, 4096, dtype=torch.bfloat16, device="cuda")
    shards = ["w.tp0", "w.tp1", "w.tp2", "w.tp3"]                                       # each (4096, 1024)
    _, statuses = read_files_device(image, names=shards, planes="manifest", place={nm: (w, 1, 1024 * r) for r, nm in enumerate(shards)})

With base= and inplace=True the destination is its own base: the previous checkpoint in the merged layout becomes the new one.

The library works with the devices of ZPACK_AMD_DEVICES (default: ZPACK_AMD_DEVICE, else LOCAL_RANK, else 0); tensors on another device
are ZPACK_ERROR_NOT_AVAILABLE.
"""
import ctypes as C
import os

from . import ZPACK_SO, METHOD_NONE, METHOD_ZSTD, METHOD_LZ4            # noqa: F401  (the methods are part of this module's interface)

OK, BUFFER_TOO_SMALL, STREAM_INVALID, NOT_AVAILABLE = 0, 12, 21, 24     # enum zpack_result (include/zpack.h)
BASE_MISMATCH = 64                                                      # ZPACK_AMD_ERROR_BASE_MISMATCH (include/zpack_amd.h): the entry's base is not the one it was written against
PLANES_MANIFEST = ".zpack_amd/planes.json"                              # the entry write_*(planes="dtype") appends: {name: element size}
DELTA_MANIFEST = ".zpack_amd/delta.json"                                # ... and with base=: {"entries": [names], "base_id": string or null, "base_xxh3": {name: 16 hex digits}}


class FileEntry(C.Structure):                # zpack_file_entry (include/zpack.h)
    _fields_ = [("filename", C.c_char_p), ("offset", C.c_uint64), ("comp_size", C.c_uint64),
                ("uncomp_size", C.c_uint64), ("hash", C.c_uint64), ("comp_method", C.c_uint8)]


class Reader(C.Structure):                   # zpack_reader
    _fields_ = [("version", C.c_uint16), ("file_entries", C.POINTER(FileEntry)), ("file_count", C.c_uint64),
                ("comp_size", C.c_uint64), ("uncomp_size", C.c_uint64), ("file_size", C.c_size_t),
                ("zstd_dctx", C.c_void_p), ("lz4f_dctx", C.c_void_p), ("last_return", C.c_size_t),
                ("cdr_offset", C.c_uint64), ("eocdr_offset", C.c_uint64), ("buffer", C.c_void_p),
                ("buffer_shared", C.c_uint8), ("file", C.c_void_p)]


class CompressOptions(C.Structure):          # zpack_compress_options
    _fields_ = [("method", C.c_int), ("level", C.c_int)]


class File(C.Structure):                     # zpack_file; `buffer` is a DEVICE address here
    _fields_ = [("filename", C.c_char_p), ("buffer", C.c_void_p), ("size", C.c_uint64),
                ("options", C.POINTER(CompressOptions)), ("cctx", C.c_void_p)]


class Writer(C.Structure):                   # zpack_writer
    _fields_ = [("buffer", C.c_void_p), ("buffer_capacity", C.c_size_t), ("file", C.c_void_p), ("file_size", C.c_size_t),
                ("write_offset", C.c_size_t), ("file_entries", C.POINTER(FileEntry)), ("fe_capacity", C.c_uint64),
                ("file_count", C.c_uint64), ("zstd_cctx", C.c_void_p), ("lz4f_cctx", C.c_void_p),
                ("last_return", C.c_size_t), ("cdr_offset", C.c_uint64), ("eocdr_offset", C.c_uint64)]


assert C.sizeof(FileEntry) == 48 and C.sizeof(Reader) == 112 and C.sizeof(File) == 40 and C.sizeof(Writer) == 104

_lib = None


def lib():
    """libzpack_amd.so with the prototypes this module uses; raises when the library is missing (there is no fallback)"""
    global _lib
    if _lib is None:
        if not os.path.exists(ZPACK_SO):
            raise RuntimeError("%s is missing: run `python -m zpack_amd.build`; there is no CPU fallback" % ZPACK_SO)
        import torch  # noqa: F401  (one HIP runtime per process: torch's comes up first, see zpack_amd.lib)
        L = C.CDLL(ZPACK_SO)
        R, W, vp, u64 = C.POINTER(Reader), C.POINTER(Writer), C.c_void_p, C.c_uint64
        L.zpack_init_reader.argtypes = [R, C.c_char_p]
        L.zpack_init_reader_memory.argtypes = [R, vp, C.c_size_t]
        L.zpack_amd_init_reader_device.argtypes = [R, vp, C.c_size_t]
        L.zpack_close_reader.argtypes = [R]
        L.zpack_close_reader.restype = None
        L.zpack_amd_read_files_device.argtypes = [R, C.POINTER(C.POINTER(FileEntry)), u64, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_int), vp]
        L.zpack_amd_read_files_device_planes.argtypes = [R, C.POINTER(C.POINTER(FileEntry)), u64, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_uint8), C.POINTER(C.c_int), vp]
        L.zpack_amd_read_files_device_delta.argtypes = [R, C.POINTER(C.POINTER(FileEntry)), u64, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_uint8), C.POINTER(vp),
                                                        C.POINTER(C.c_int), vp]
        L.zpack_amd_read_files_device_delta_checked.argtypes = [R, C.POINTER(C.POINTER(FileEntry)), u64, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_uint8), C.POINTER(vp),
                                                                C.POINTER(u64), C.POINTER(C.c_int), vp]
        L.zpack_amd_read_files_device_windows.argtypes = [R, C.POINTER(C.POINTER(FileEntry)), u64, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_uint8), C.POINTER(vp),
                                                          C.POINTER(u64), C.POINTER(Window), C.POINTER(C.c_int), vp]
        L.zpack_amd_read_files_device_placed.argtypes = [R, C.POINTER(C.POINTER(FileEntry)), u64, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_uint8), C.POINTER(vp),
                                                         C.POINTER(u64), C.POINTER(Window), C.POINTER(u64), C.POINTER(C.c_int), vp]
        L.zpack_amd_hash_device.argtypes = [C.POINTER(vp), C.POINTER(C.c_size_t), u64, C.POINTER(u64), vp]
        L.zpack_read_file.argtypes = [R, C.POINTER(FileEntry), vp, C.c_size_t, vp]
        L.zpack_amd_read_files_device_packed.argtypes = [R, C.POINTER(C.POINTER(FileEntry)), u64, vp, C.c_size_t, C.POINTER(u64), C.POINTER(C.c_int), vp]
        L.zpack_amd_test_files.argtypes = [R, C.POINTER(C.POINTER(FileEntry)), u64, C.POINTER(C.c_int), vp]
        L.zpack_init_writer.argtypes = [W, C.c_char_p]
        L.zpack_init_writer_heap.argtypes = [W, C.c_size_t]
        L.zpack_amd_init_writer_device.argtypes = [W, vp, C.c_size_t]
        L.zpack_write_header.argtypes = [W]
        L.zpack_write_data_header.argtypes = [W]
        L.zpack_amd_write_files_device.argtypes = [W, C.POINTER(File), u64]
        L.zpack_amd_write_files_device_planes.argtypes = [W, C.POINTER(File), u64, C.POINTER(C.c_uint8)]
        L.zpack_amd_write_files_device_delta.argtypes = [W, C.POINTER(File), u64, C.POINTER(C.c_uint8), C.POINTER(vp)]
        L.zpack_write_files.argtypes = [W, C.POINTER(File), u64]
        L.zpack_write_cdr.argtypes = [W]
        L.zpack_write_eocdr.argtypes = [W]
        L.zpack_close_writer.argtypes = [W]
        L.zpack_close_writer.restype = None
        _lib = L
    return _lib


def _settle(device):
    """The library's codec runs on a stream of its own: what torch has enqueued for these tensors on its current stream — the fill that
    made a source, the last use of a block the allocator hands out again — has to have finished (Codec._settle documents the same)."""
    import torch
    torch.cuda.current_stream(device).synchronize()


def _check(rc, what):
    if rc != OK:
        raise RuntimeError("%s -> %d%s" % (what, rc, " (no usable HIP device, or tensors on a device outside ZPACK_AMD_DEVICES: there is no CPU fallback)"
                                                 if rc == NOT_AVAILABLE else ""))


def _open_reader(L, r, archive, device):
    """Opens `r` over `archive` — a path, the archive's bytes, or the image as a contiguous uint8 CUDA tensor — and returns the device the
    call works with (the tensor's for an image); the caller closes the reader"""
    import torch
    if isinstance(archive, torch.Tensor):
        if not (archive.is_cuda and archive.dtype == torch.uint8 and archive.dim() == 1 and archive.is_contiguous()):
            raise ValueError("an archive image in device memory is a contiguous one-dimensional uint8 CUDA tensor")
        device = archive.device.index
        _settle(archive.device)                                                     # whatever filled the image has finished
        _check(L.zpack_amd_init_reader_device(C.byref(r), archive.data_ptr(), archive.numel()), "zpack_amd_init_reader_device")
    elif isinstance(archive, (str, os.PathLike)):
        _check(L.zpack_init_reader(C.byref(r), os.fsencode(archive)), "zpack_init_reader")
    else:
        raw = bytes(archive)
        _check(L.zpack_init_reader_memory(C.byref(r), raw, len(raw)), "zpack_init_reader_memory")
    return device


def _picks(r, names):
    """the entries `names` of an opened reader, in that order (None: all, in archive order), as indices into its table"""
    if names is None:
        return list(range(r.file_count))
    first = {}
    for i in range(r.file_count):
        first.setdefault(r.file_entries[i].filename.decode(), i)
    return [first[n] for n in names]                                                # KeyError: no such entry


def test_files(archive, names=None, device=0):
    """The verdicts of read_files_device without the tensors (zpack_amd_test_files): every entry is decoded and hashed on the device and
    nothing but descriptors and results crosses the bus — for an image in device memory not even the compressed bytes.  `archive` and
    `names` as in read_files_device; no tensor is allocated.  Returns the zpack_result of each entry (0 = decoded and its XXH3 verified)."""
    L = lib()
    r = Reader()
    _open_reader(L, r, archive, device)
    try:
        picks = _picks(r, names)
        n = len(picks)
        ents = (C.POINTER(FileEntry) * max(n, 1))(*[C.pointer(r.file_entries[i]) for i in picks])
        res = (C.c_int * max(n, 1))()
        _check(L.zpack_amd_test_files(C.byref(r), ents, n, res, None), "zpack_amd_test_files")
        return [int(res[i]) for i in range(n)]
    finally:
        L.zpack_close_reader(C.byref(r))


test_files.__test__ = False                     # (a library function, not a test: pytest collects nothing here)


def _read_json_entry(L, r, name, valid, what):
    """the JSON value of the opened reader's entry `name`, read through the host call; None when there is no such entry; raises when it
    does not parse or valid(value) is false (`what` says what it should have been)"""
    import json
    for i in range(r.file_count):
        e = r.file_entries[i]
        if e.filename.decode() != name:
            continue
        raw = C.create_string_buffer(max(int(e.uncomp_size), 1))
        _check(L.zpack_read_file(C.byref(r), C.pointer(e), raw, int(e.uncomp_size), None), "zpack_read_file(%s)" % name)
        try:
            m = json.loads(raw.raw[:int(e.uncomp_size)].decode())
            if not valid(m):
                raise ValueError("not %s" % what)
        except ValueError as err:                                                   # (json's and unicode's errors are ValueErrors)
            raise ValueError("%s does not parse: %s" % (name, err)) from None
        return m
    return None


def _read_manifest(L, r):
    """the {name: element size} map of the opened reader's PLANES_MANIFEST entry; raises when there is none or it does not parse"""
    m = _read_json_entry(L, r, PLANES_MANIFEST, lambda m: isinstance(m, dict) and all(isinstance(k, str) and v in (1, 2, 4, 8) and not isinstance(v, bool)
                                                                                    for k, v in m.items()), "a {name: 1 | 2 | 4 | 8} map")
    if m is None:
        raise KeyError("the archive has no %s entry: it was not written with planes=\"dtype\"" % PLANES_MANIFEST)
    return m


def _delta_manifest_valid(m):
    """DELTA_MANIFEST as the writers write it; "base_xxh3" may be missing (archives from before the bases were hashed), but when it is
    there it is {name: 16 lower-case hex digits} for exactly the names listed under "entries".  A plain function of the parsed JSON."""
    if not (isinstance(m, dict) and isinstance(m.get("entries"), list) and all(isinstance(k, str) for k in m["entries"])
            and (m.get("base_id") is None or isinstance(m["base_id"], str))):
        return False
    if "base_xxh3" not in m:
        return True
    h = m["base_xxh3"]
    return (isinstance(h, dict) and set(h) == set(m["entries"])
            and all(isinstance(v, str) and len(v) == 16 and all(ch in "0123456789abcdef" for ch in v) for v in h.values()))


def _parse_delta_manifest(m):
    """(names of the delta entries, recorded base_id or None, {name: the base's XXH3-64} or None) of DELTA_MANIFEST's value; None: no manifest"""
    if m is None:
        return [], None, None
    hashes = m.get("base_xxh3")
    return m["entries"], m.get("base_id"), None if hashes is None else {k: int(v, 16) for k, v in hashes.items()}


def _read_delta_manifest(L, r):
    """_parse_delta_manifest of the opened reader's DELTA_MANIFEST entry; raises when it does not parse"""
    return _parse_delta_manifest(_read_json_entry(L, r, DELTA_MANIFEST, _delta_manifest_valid,
                                                  "{\"entries\": [names], \"base_id\": string or null, \"base_xxh3\": {name: 16 hex digits}}"))


def _hash_flat(L, flats):
    """XXH3-64 of flat uint8 CUDA tensors, hashed where they lie (zpack_amd_hash_device), as ints"""
    n = len(flats)
    if n == 0:
        return []
    for d in set(t.device for t in flats):
        _settle(d)
    ptrs = (C.c_void_p * n)(*[t.data_ptr() if t.numel() else None for t in flats])
    sizes = (C.c_size_t * n)(*[t.numel() for t in flats])
    out = (C.c_uint64 * n)()
    _check(L.zpack_amd_hash_device(ptrs, sizes, n, out, None), "zpack_amd_hash_device")
    return [int(out[i]) for i in range(n)]


def hash_tensors(tensors):
    """The XXH3-64 (seed 0) of each tensor's bytes in memory order, computed on the device (zpack_amd_hash_device): the value an archive
    records as `hash` for an entry with those plain bytes, and the value DELTA_MANIFEST records for a base.  `tensors`: {name: CUDA
    tensor} -> {name: int}, or a sequence of CUDA tensors -> [int].  All on one device; nothing but the hashes crosses the bus."""
    if isinstance(tensors, dict):
        _, flat = _flatten(tensors, "hash_tensors")
        return dict(zip(tensors.keys(), _hash_flat(lib(), flat)))
    _, flat = _flatten({str(i): t for i, t in enumerate(tensors)}, "hash_tensors")
    return _hash_flat(lib(), flat)


def _base_bytes(name, t, size):
    """the base tensor of entry `name` as its bytes in memory order — a view, never a copy: it may be the destination"""
    if not (t.is_cuda and t.is_contiguous()):
        raise ValueError("the base of %s is a contiguous CUDA tensor" % name)
    flat = t.reshape(-1).view(dtype=_u8())
    if flat.numel() != size:
        raise ValueError("the base of %s has %d bytes, the entry %d" % (name, flat.numel(), size))
    return flat


class Window(C.Structure):                   # zpack_amd_window (include/zpack_amd.h)
    _fields_ = [("row_bytes", C.c_uint64), ("row0", C.c_uint64), ("rows", C.c_uint64), ("col0", C.c_uint64), ("cols", C.c_uint64)]


def _windows_of(pnames, sizes, planes, window):
    """the `window` argument of read_files_device as one Window per entry read (row_bytes 0: the entry whole), or None when no entry has
    one; ValueError naming the entry for a shape that does not multiply out to its size or a dim, start or stop out of range"""
    from . import slice_window
    if not window:
        return None
    unknown = [nm for nm in window if nm not in pnames]
    if unknown:
        raise KeyError("window names no entry of this read: %s" % ", ".join(unknown))
    out = []
    for nm, size in zip(pnames, sizes):
        if nm not in window:
            out.append(Window(0, 0, 0, 0, 0))
            continue
        try:
            shape, dim, start, stop = window[nm]
            shape, dim, start, stop = [int(x) for x in shape], int(dim), int(start), int(stop)
            k = int(planes.get(nm, 1)) if planes else 1
            count = 1
            for x in shape:
                count *= x
            if not shape or any(x < 0 for x in shape) or count * k != size:
                raise ValueError("shape %r of %d-byte elements is not its %d bytes" % (tuple(shape), k, size))
            out.append(Window(*slice_window(shape, dim, start, stop, k)))
        except (TypeError, ValueError) as err:
            raise ValueError("window of %s: %s" % (nm, err)) from None
    return out


def _places_of(pnames, sizes, wins, place, dev):
    """the `place` argument of read_files_device against the entries read: (wins, pitches, offsets, extents) — the windows with one for
    every placed entry (an entry placed whole becomes the window that is all of it), its pitch (0: not placed), the byte offset of its
    sub-block in its destination tensor and the bytes from that offset to the sub-block's last; ValueError naming the entry for a
    destination that is not a contiguous tensor on `dev`, a size that does not divide into the destination's rows, or a slice past it"""
    from . import place_of
    unknown = [nm for nm in place if nm not in pnames]
    if unknown:
        raise KeyError("place names no entry of this read: %s" % ", ".join(unknown))
    wins = list(wins) if wins is not None else [Window(0, 0, 0, 0, 0) for _ in pnames]
    pitches, offsets, extents = [0] * len(pnames), [0] * len(pnames), [0] * len(pnames)
    for k, (nm, size) in enumerate(zip(pnames, sizes)):
        if nm not in place:
            continue
        try:
            dest, dim, start = place[nm]
            dim, start = int(dim), int(start)
            if not (dest.is_cuda and dest.is_contiguous() and dest.device == dev):
                raise ValueError("the destination is a contiguous CUDA tensor on %s" % (dev,))
            w = wins[k]
            n = int(w.rows * w.cols) if w.row_bytes else size                           # the bytes delivered
            rows, unit, pitch, _ = place_of(dest.shape, dim, 0, 1, dest.element_size())   # (unit: the bytes of one step along dim, in one row)
            if rows * unit == 0 or n % (rows * unit):
                raise ValueError("%d bytes do not divide into %d rows of %d-byte steps along dim %d of %r" % (n, rows, unit, dim, tuple(dest.shape)))
            rows, cols, pitch, offset = place_of(dest.shape, dim, start, n // (rows * unit), dest.element_size())
            if n == 0:
                continue                                                                # (nothing to deliver: no placement)
            if not w.row_bytes:
                w = Window(cols, 0, rows, 0, cols)                                      # the entry whole, seen as the sub-block's rows
            elif (w.rows, w.cols) != (rows, cols):
                # a window that is one contiguous run of the entry (whole rows, or part of one row) is that run seen as the sub-block's rows
                first = w.row0 * w.row_bytes + w.col0
                if not (w.rows == 1 or w.cols == w.row_bytes) or first % cols or size % cols:
                    raise ValueError("its window has %d rows of %d bytes, the destination %d of %d" % (w.rows, w.cols, rows, cols))
                w = Window(cols, first // cols, rows, 0, cols)
            wins[k], pitches[k], offsets[k], extents[k] = w, pitch, offset, (rows - 1) * pitch + cols
        except (TypeError, ValueError) as err:
            raise ValueError("place of %s: %s" % (nm, err)) from None
    return wins, pitches, offsets, extents


def read_files_device(archive, names=None, device=0, planes=None, base=None, inplace=False, base_id=None, check_base=True, window=None, place=None):
    """`archive`: a path, the archive's bytes, or the archive image as a contiguous uint8 CUDA tensor (zpack_amd_init_reader_device: the
    compressed bytes are decoded where they lie, nothing crosses the bus; `device` is then the tensor's).  `names`: the entries to read,
    in that order (None: all, in archive order).  `planes`: None — the entries' bytes as they are stored; {name: element size} — those
    entries are byte-plane entries and come back joined (names left out: 1); "manifest" — the map is the archive's PLANES_MANIFEST entry
    (raises when that is missing or does not parse), and with names None that entry is left out of what is returned.
    `base`: {name: CUDA tensor of the entry's size} — those entries are delta entries and come back XORed with their base (the module's
    docstring); inplace=True: the base tensors are the destinations and are what is returned for their entries — an entry that does not
    decode leaves its base as it was.  With planes="manifest" the archive's DELTA_MANIFEST says which entries are delta entries: one
    of those among the entries read without a base raises KeyError naming it (its bytes alone are not the tensor), and a `base_id`
    that differs from the recorded one raises ValueError; with names None that entry is left out too.  When the manifest records the
    bases' hashes ("base_xxh3") the bases given are hashed on the device before they are applied: an entry whose base is another comes back
    with status BASE_MISMATCH, its tensor — with inplace=True its base — untouched; check_base=False reads without that check, as an
    archive without the field is read.
    `window`: {name: (shape, dim, start, stop)} — of those entries only the slice [start, stop) along dimension `dim` of the entry seen
    as a contiguous tensor of `shape` is delivered (zpack_amd_read_files_device_windows: the cut rides on the copy that delivers the
    entry, no full-size tensor is allocated); `shape` counts elements of the entry's element size, its `planes` value or 1.  The tensor
    returned for such an entry has the slice's bytes, and its base — with inplace=True the destination, as ever — is the caller's shard of
    that size.  A shape that does not multiply out to the entry's size, or a dim, start or stop out of range, raises ValueError naming
    the entry before anything is decoded.  A recorded "base_xxh3" is the hash of the WHOLE base, which the reader of a window does not
    hold: a windowed entry with a base in such an archive raises ValueError unless check_base=False.  None: no entry has a window.
    `place`: {name: (dest_tensor, dim, start)} — those entries, or their `window` slices, land at [start, start + length) along dimension
    `dim` of the caller's contiguous `dest_tensor` on the read's device (zpack_amd_read_files_device_placed: the placement rides on the
    copy that delivers the entry; several entries may share one destination, side by side).  `length` follows from the entry's size —
    the bytes delivered over the destination's rows and the bytes of one step along `dim`; a size that does not divide, or a slice past
    the destination, raises ValueError naming the entry before anything is decoded.  The tensor returned for such an entry is
    `dest_tensor`; what the read does not place in it stays as it was.  Its base is a tensor in the destination's layout and of its
    size, read at the bytes that are written; with inplace=True it is `dest_tensor` itself: the destination is its own base.  A recorded
    "base_xxh3" is handled as for a windowed entry: ValueError unless check_base=False.  None: no entry is placed.
    Returns (tensors, statuses): one uint8 CUDA tensor of uncomp_size bytes per entry on cuda:`device` — views of one allocation, each at
    a multiple of 256 — and the zpack_result of each (0 = decoded and its XXH3 verified; anything else: the tensor's bytes are not the entry)."""
    import torch
    L = lib()
    r = Reader()
    device = _open_reader(L, r, archive, device)
    try:
        picks = _picks(r, names)
        base = dict(base or {})
        recorded_hash = None
        if planes == "manifest":
            planes = _read_manifest(L, r)
            delta_names, recorded_id, recorded_hash = _read_delta_manifest(L, r)
            if names is None:
                picks = [i for i in picks if r.file_entries[i].filename.decode() not in (PLANES_MANIFEST, DELTA_MANIFEST)]
            if base_id is not None and base_id != recorded_id:
                raise ValueError("the archive's entries are deltas against base %r, not %r" % (recorded_id, base_id))
            picked = set(r.file_entries[i].filename.decode() for i in picks)
            for name in delta_names:
                if name in picked and name not in base:
                    raise KeyError("%s is a delta entry: read_files_device needs base[%r]" % (name, name))
        elif planes is not None and not isinstance(planes, dict):
            raise ValueError("planes is None, a {name: element size} dict or \"manifest\"")
        n = len(picks)
        sizes = [int(r.file_entries[i].uncomp_size) for i in picks]
        pnames = [r.file_entries[i].filename.decode() for i in picks]
        wins = _windows_of(pnames, sizes, planes, window)
        if wins is not None:
            for nm, w in zip(pnames, wins):
                if w.row_bytes and nm in base and check_base and recorded_hash is not None:
                    raise ValueError("%s: the archive records the hash of its WHOLE base, which the reader of a window does not hold; read it with check_base=False" % nm)
            sizes = [int(w.rows * w.cols) if w.row_bytes else s for w, s in zip(wins, sizes)]      # (what the buffers and the bases hold)
        dev = torch.device("cuda", device)
        pitches = None
        if place:
            whole = [int(r.file_entries[i].uncomp_size) for i in picks]
            wins, pitches, offsets, extents = _places_of(pnames, whole, wins, place, dev)
            for k, nm in enumerate(pnames):
                if pitches[k] and nm in base and check_base and recorded_hash is not None:
                    raise ValueError("%s: the archive records the hash of its base as one span, which a placed base is not; read it with check_base=False" % nm)
            sizes = [0 if p else s for p, s in zip(pitches, sizes)]                                # (a placed entry takes nothing of the backing)
        starts, total = [], 0
        for s in sizes:
            starts.append(total)
            total += (s + 255) & ~255
        backing = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        tensors = [backing[a:a + s] for a, s in zip(starts, sizes)]
        bases = [_base_bytes(nm, base[nm], s) if nm in base and not (pitches and pitches[k]) else None for k, (nm, s) in enumerate(zip(pnames, sizes))]
        out = list(tensors)
        if inplace:
            for k, b in enumerate(bases):
                if b is not None:
                    tensors[k], out[k] = b, base[pnames[k]]
        if pitches:
            # a placed entry: its buffer is its sub-block of the destination, its base the same bytes of a tensor in the destination's layout
            for k, nm in enumerate(pnames):
                if not pitches[k]:
                    continue
                dest = place[nm][0]
                flat = dest.reshape(-1).view(dtype=_u8())
                tensors[k], out[k], sizes[k] = flat[offsets[k]:offsets[k] + extents[k]], dest, extents[k]
                if nm in base:
                    b = _base_bytes(nm, base[nm], flat.numel())
                    if inplace and b.data_ptr() != flat.data_ptr():
                        raise ValueError("place of %s: with inplace=True the destination is its own base" % nm)
                    bases[k] = b[offsets[k]:offsets[k] + extents[k]]
        ents = (C.POINTER(FileEntry) * max(n, 1))(*[C.pointer(r.file_entries[i]) for i in picks])
        bufs = (C.c_void_p * max(n, 1))(*[t.data_ptr() if s else None for t, s in zip(tensors, sizes)])
        caps = (C.c_size_t * max(n, 1))(*sizes)
        res = (C.c_int * max(n, 1))()
        _settle(dev)
        elem = None if planes is None else (C.c_uint8 * max(n, 1))(*[int(planes.get(nm, 1)) for nm in pnames])
        if wins is not None:
            d_bases = want = None
            if any(b is not None for b in bases):
                for b in bases:
                    if b is not None:
                        _settle(b.device)
                d_bases = (C.c_void_p * max(n, 1))(*[b.data_ptr() if b is not None and b.numel() else None for b in bases])
                if check_base and recorded_hash is not None:                        # (no windowed entry has a base here: the entries read whole are checked as ever)
                    unlisted = [k for k, (nm, b) in enumerate(zip(pnames, bases)) if b is not None and nm not in recorded_hash]
                    own = dict(zip(unlisted, _hash_flat(L, [bases[k] for k in unlisted])))
                    want = (C.c_uint64 * max(n, 1))(*[own[k] if k in own else recorded_hash.get(nm, 0) for k, nm in enumerate(pnames)])
            if pitches:
                _check(L.zpack_amd_read_files_device_placed(C.byref(r), ents, n, bufs, caps, elem, d_bases, want, (Window * max(n, 1))(*wins),
                                                            (C.c_uint64 * max(n, 1))(*pitches), res, None), "zpack_amd_read_files_device_placed")
            else:
                _check(L.zpack_amd_read_files_device_windows(C.byref(r), ents, n, bufs, caps, elem, d_bases, want, (Window * max(n, 1))(*wins), res, None),
                       "zpack_amd_read_files_device_windows")
        elif any(b is not None for b in bases):
            for b in bases:
                if b is not None:
                    _settle(b.device)
            d_bases = (C.c_void_p * max(n, 1))(*[b.data_ptr() if b is not None and b.numel() else None for b in bases])
            if check_base and recorded_hash is not None:
                # (a base given for an entry the manifest does not list has no recorded value: its own hash, which passes)
                unlisted = [k for k, (nm, b) in enumerate(zip(pnames, bases)) if b is not None and nm not in recorded_hash]
                own = dict(zip(unlisted, _hash_flat(L, [bases[k] for k in unlisted])))
                want = (C.c_uint64 * max(n, 1))(*[own[k] if k in own else recorded_hash.get(nm, 0) for k, nm in enumerate(pnames)])
                _check(L.zpack_amd_read_files_device_delta_checked(C.byref(r), ents, n, bufs, caps, elem, d_bases, want, res, None),
                       "zpack_amd_read_files_device_delta_checked")
            else:
                _check(L.zpack_amd_read_files_device_delta(C.byref(r), ents, n, bufs, caps, elem, d_bases, res, None), "zpack_amd_read_files_device_delta")
        elif planes is None:
            _check(L.zpack_amd_read_files_device(C.byref(r), ents, n, bufs, caps, res, None), "zpack_amd_read_files_device")
        else:
            _check(L.zpack_amd_read_files_device_planes(C.byref(r), ents, n, bufs, caps, elem, res, None), "zpack_amd_read_files_device_planes")
        return out, [int(res[i]) for i in range(n)]
    finally:
        L.zpack_close_reader(C.byref(r))


def _flatten(tensors, who):
    """{name: CUDA tensor} as ([(name, tensor)], [its bytes in memory order as a flat uint8 tensor])"""
    items = list(tensors.items())
    flat = [t.contiguous().reshape(-1).view(dtype=_u8()) for _, t in items]
    for t in flat:
        if not t.is_cuda:
            raise ValueError("%s takes CUDA tensors (zpack_write_files is the call for host memory)" % who)
    return items, flat


def _elem_sizes(items, planes):
    """(element size per item or None, the manifest's bytes or None) for the `planes` argument of the writers"""
    import json
    if planes is None:
        return None, None
    if isinstance(planes, dict):
        return [int(planes.get(name, 1)) for name, _ in items], None
    if planes != "dtype":
        raise ValueError("planes is None, a {name: element size} dict or \"dtype\"")
    if any(name == PLANES_MANIFEST for name, _ in items):
        raise ValueError("%s is the name of the manifest planes=\"dtype\" writes" % PLANES_MANIFEST)
    elem = [t.element_size() if t.dtype.is_floating_point and t.element_size() in (2, 4, 8) else 1 for _, t in items]
    return elem, json.dumps({name: k for (name, _), k in zip(items, elem)}, separators=(",", ":")).encode()


def _bases_of(items, flat, base, base_id, with_manifest, check_base=False):
    """(the base's bytes per item or None — None when no item has one —, DELTA_MANIFEST's bytes or None) for the `base` argument of the writers;
    check_base: the manifest also records the bases' XXH3-64, hashed on the device ("base_xxh3")"""
    import json
    if not base:
        return None, None
    unknown = [name for name in base if name not in dict(items)]
    if unknown:
        raise KeyError("base names no tensor of this call: %s" % ", ".join(unknown))
    if base_id is not None and not isinstance(base_id, str):
        raise ValueError("base_id is a string")
    bases = [_base_bytes(name, base[name], t.numel()) if name in base else None for (name, _), t in zip(items, flat)]
    if not with_manifest:
        return bases, None
    if any(name == DELTA_MANIFEST for name, _ in items):
        raise ValueError("%s is the name of the manifest base= writes" % DELTA_MANIFEST)
    listed = [(name, b) for (name, _), b in zip(items, bases) if b is not None]
    m = {"entries": [name for name, _ in listed], "base_id": base_id}
    if check_base:
        hashes = _hash_flat(lib(), [b for _, b in listed])                            # on the device, where the bases lie
        m["base_xxh3"] = {name: "%016x" % h for (name, _), h in zip(listed, hashes)}
    return bases, json.dumps(m, separators=(",", ":")).encode()


def _write_archive(L, w, items, flat, method, level, elem=None, manifest=None, bases=None, delta_manifest=None):
    """The body both writers share: header, data signature, the entries out of device memory (elem: their element sizes, byte planes;
    bases: what they are XORed with, delta entries), the manifests as stored entries out of host memory, CDR and EOCDR into the opened
    writer `w`"""
    opts = CompressOptions(int(method), int(level))
    arr = (File * max(len(items), 1))()
    for i, ((name, _), t) in enumerate(zip(items, flat)):
        arr[i].filename = name.encode()
        arr[i].buffer = t.data_ptr() if t.numel() else None
        arr[i].size = t.numel()
        arr[i].options = C.pointer(opts)
        arr[i].cctx = None
    _check(L.zpack_write_header(C.byref(w)), "zpack_write_header")
    _check(L.zpack_write_data_header(C.byref(w)), "zpack_write_data_header")
    c_elem = None if elem is None else (C.c_uint8 * max(len(items), 1))(*elem)
    if bases is not None:
        for b in bases:
            if b is not None:
                _settle(b.device)
        d_bases = (C.c_void_p * max(len(items), 1))(*[b.data_ptr() if b is not None and b.numel() else None for b in bases])
        _check(L.zpack_amd_write_files_device_delta(C.byref(w), arr, len(items), c_elem, d_bases), "zpack_amd_write_files_device_delta")
    elif elem is None:
        _check(L.zpack_amd_write_files_device(C.byref(w), arr, len(items)), "zpack_amd_write_files_device")
    else:
        _check(L.zpack_amd_write_files_device_planes(C.byref(w), arr, len(items), c_elem), "zpack_amd_write_files_device_planes")
    for mname, mbytes in ((PLANES_MANIFEST, manifest), (DELTA_MANIFEST, delta_manifest)):
        if mbytes is None:
            continue
        stored = CompressOptions(int(METHOD_NONE), 0)
        raw = C.create_string_buffer(mbytes, len(mbytes))
        one = (File * 1)()
        one[0].filename = mname.encode()
        one[0].buffer = C.cast(raw, C.c_void_p)
        one[0].size = len(mbytes)
        one[0].options = C.pointer(stored)
        one[0].cctx = None
        _check(L.zpack_write_files(C.byref(w), one, 1), "zpack_write_files(%s)" % mname)
    _check(L.zpack_write_cdr(C.byref(w)), "zpack_write_cdr")
    _check(L.zpack_write_eocdr(C.byref(w)), "zpack_write_eocdr")


def write_files_device(path, tensors, method=METHOD_LZ4, level=0, planes=None, base=None, base_id=None, check_base=False):
    """Writes the archive `path` with one entry per item of `tensors` ({name: CUDA tensor}, all on one device; any dtype: an entry is the
    tensor's bytes in memory order).  path None: the archive is built on the heap and returned as bytes.  `planes`: None — the bytes as
    they are; {name: element size} — those entries are stored as byte planes; "dtype" — the element size of every floating tensor of 2,
    4 or 8 bytes an element, and the PLANES_MANIFEST entry behind the tensors' (the module's docstring).  `base`: {name: CUDA tensor
    with the nbytes of tensors[name]} — those entries are stored as deltas against it; with planes="dtype" the DELTA_MANIFEST entry
    records their names and `base_id`, a string of the caller's that names the base (None: none).  check_base=True: the bases are
    hashed on the device and DELTA_MANIFEST also records "base_xxh3", which makes read_files_device refuse any other base (the
    module's docstring); the default writes the manifest as it always was."""
    L = lib()
    items, flat = _flatten(tensors, "write_files_device")
    elem, manifest = _elem_sizes(items, planes)
    bases, delta_manifest = _bases_of(items, flat, base, base_id, manifest is not None, check_base)
    w = Writer()
    _check(L.zpack_init_writer(C.byref(w), os.fsencode(path)) if path is not None else L.zpack_init_writer_heap(C.byref(w), 0), "zpack_init_writer")
    try:
        if flat:
            _settle(flat[0].device)
        _write_archive(L, w, items, flat, method, level, elem, manifest, bases, delta_manifest)
        return C.string_at(w.buffer, w.file_size) if path is None else None
    finally:
        L.zpack_close_writer(C.byref(w))


def archive_capacity(sizes, names, method):
    """Bytes that hold any archive of entries of `sizes` bytes named `names`, compressed with `method`: header (6) and data signature (4),
    the compress bounds, the CDR (20 + 35 + the name's length per entry) and the EOCDR (12)."""
    from . import lib as codec_lib
    bound = codec_lib().zpk_codec_compress_bound
    return 10 + sum(int(bound(int(method), int(s))) for s in sizes) + 20 + sum(35 + len(n.encode()) for n in names) + 12


def write_archive_device(tensors, method=METHOD_LZ4, level=0, capacity=None, planes=None, base=None, base_id=None, check_base=False):
    """Writes an archive with one entry per item of `tensors` ({name: CUDA tensor}, all on one device) INTO DEVICE MEMORY
    (zpack_amd_init_writer_device): header, files, CDR and EOCDR go into a fresh uint8 tensor of `capacity` bytes on the tensors' device
    (None: archive_capacity, which holds whatever the entries compress to), the frames are committed there by the codec's kernels and no
    compressed byte crosses the bus.  Returns the tensor trimmed to the archive's size; it is byte for byte what write_files_device
    returns for path None.  A capacity that is too small raises (ZPACK_ERROR_BUFFER_TOO_SMALL, 12).  `planes`, `base`, `base_id`,
    `check_base`: as in write_files_device.

        image = write_archive_device({"a": ta, "b": tb}, method=METHOD_ZSTD, level=1)
        tensors, statuses = read_files_device(image)                      # zpack_amd_init_reader_device: read where it was written
    """
    import torch
    L = lib()
    items, flat = _flatten(tensors, "write_archive_device")
    elem, manifest = _elem_sizes(items, planes)
    bases, delta_manifest = _bases_of(items, flat, base, base_id, manifest is not None, check_base)
    dev = flat[0].device if flat else torch.device("cuda", 0)
    if capacity is None:
        capacity = archive_capacity([t.numel() for t in flat], [name for name, _ in items], method)
        if manifest is not None:                                                    # (a stored entry: its bound is its size)
            capacity += archive_capacity([len(manifest)], [PLANES_MANIFEST], METHOD_NONE) - 42
        if delta_manifest is not None:
            capacity += archive_capacity([len(delta_manifest)], [DELTA_MANIFEST], METHOD_NONE) - 42
    image = torch.empty(max(int(capacity), 1), dtype=torch.uint8, device=dev)
    w = Writer()
    _settle(dev)
    _check(L.zpack_amd_init_writer_device(C.byref(w), image.data_ptr(), int(capacity)), "zpack_amd_init_writer_device")
    try:
        _write_archive(L, w, items, flat, method, level, elem, manifest, bases, delta_manifest)
        return image[:int(w.file_size)]
    finally:
        L.zpack_close_writer(C.byref(w))


def _u8():
    import torch
    return torch.uint8
