"""GPU: the torch view of the base check (zpack_amd/device_io.py).  Writers with base= and check_base=True hash the bases on the device and record them in
DELTA_MANIFEST; read_files_device(..., planes="manifest", base=...) hashes the bases it is given before it applies them: the right base
reads as ever, a base one optimizer step off comes back BASE_MISMATCH with its tensor untouched, an archive from before the field reads
as it did.  hash_tensors gives the `hash` field of the same tensors written as plain entries."""
import json

import numpy as np
import pytest

from zpack_amd import device_io
from tests import zpk
from tests._libs import oracle, METHOD_ZSTD, METHOD_LZ4
from tests.device_mem import torch      # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

OK = 0


def _bytes(t):
    return t.contiguous().view(-1).view(dtype=device_io._u8()).cpu().numpy().copy()


@pytest.fixture(scope="module")
def ckpt(torch):
    """step 0 (`old`), step 1 (`new`: one weight of sixteen moves a little) and step 1 after one more optimizer update (`off`)"""
    g = torch.Generator().manual_seed(30)
    old = {
        "w.bf16": (torch.randn(300, 70, generator=g) * 0.02).to(torch.bfloat16).to("cuda:0"),
        "w.fp32": (torch.randn(65537, generator=g) * 0.02).to("cuda:0"),
        "ids.int64": torch.arange(1000, dtype=torch.int64, device="cuda:0"),
    }

    def step(ts, factor):
        out = {k: t.clone() for k, t in ts.items()}
        for k in ("w.bf16", "w.fp32"):
            flat = out[k].view(-1)
            flat[::16] = (flat[::16].float() * factor).to(flat.dtype)
        out["ids.int64"] += 1
        return out

    new = step(old, 1.01)
    new["fresh.fp32"] = (torch.randn(129, generator=g) * 0.02).to("cuda:0")             # not in the previous checkpoint: no base
    off = step(old, 1.02)                                                               # the buffers of `old` after another update: same sizes, other bytes
    torch.cuda.synchronize()
    return dict(old=old, new=new, off=off)


@pytest.mark.parametrize("mc", [pytest.param((METHOD_LZ4, 0), id="lz4"), pytest.param((METHOD_ZSTD, 1), id="zstd1")])
def test_the_right_base_reads_a_base_one_step_off_is_refused_and_an_older_manifest_reads_as_ever(torch, ckpt, mc):
    old, new, off = ckpt["old"], ckpt["new"], ckpt["off"]
    raw = {k: _bytes(t) for k, t in new.items()}
    image = device_io.write_archive_device(new, method=mc[0], level=mc[1], planes="dtype", base=old, base_id="step 0", check_base=True)
    assert device_io.write_files_device(None, new, method=mc[0], level=mc[1], planes="dtype", base=old, base_id="step 0", check_base=True) == image.cpu().numpy().tobytes()
    # the manifest: the two fields it had and the bases' hashes, which are the CPU XXH3 of the bases' bytes
    outs, status = device_io.read_files_device(image)
    assert status == [OK] * (len(new) + 2)
    manifest = json.loads(outs[-1].cpu().numpy().tobytes().decode())
    o = oracle()
    assert manifest == {"entries": list(old), "base_id": "step 0", "base_xxh3": {k: "%016x" % o.xxh3(_bytes(t).tobytes()) for k, t in old.items()}}
    assert device_io.hash_tensors(old) == {k: int(v, 16) for k, v in manifest["base_xxh3"].items()}
    # the right base: fresh tensors, then in place into copies of the base
    for archive in (image, image.cpu().numpy().tobytes()):
        outs, status = device_io.read_files_device(archive, planes="manifest", base=old, base_id="step 0")
        assert status == [OK] * len(new)
        for name, got in zip(new, outs):
            assert np.array_equal(got.cpu().numpy(), raw[name]), name
    mine = {k: t.clone() for k, t in old.items()}
    outs, status = device_io.read_files_device(image, planes="manifest", base=mine, inplace=True)
    assert status == [OK] * len(new) and all(torch.equal(mine[k], new[k]) for k in old)
    # a base one optimizer step off: every entry with a base is refused and its tensor is untouched; the entry without a base is read
    for archive in (image, image.cpu().numpy().tobytes()):
        theirs = {k: t.clone() for k, t in off.items()}
        before = {k: _bytes(t) for k, t in theirs.items()}
        outs, status = device_io.read_files_device(archive, planes="manifest", base=theirs, base_id="step 0", inplace=True)
        assert status == [device_io.BASE_MISMATCH] * 3 + [OK]
        for k in old:
            assert outs[list(new).index(k)] is theirs[k] and np.array_equal(_bytes(theirs[k]), before[k]), k      # the previous checkpoint survives, bit for bit
        assert np.array_equal(outs[3].cpu().numpy(), raw["fresh.fp32"])
        # ... one wrong base among right ones, into fresh tensors: that entry alone
        mixed = dict(old, **{"w.fp32": off["w.fp32"]})
        outs, status = device_io.read_files_device(archive, planes="manifest", base=mixed)
        assert status == [OK, device_io.BASE_MISMATCH, OK, OK]
        assert np.array_equal(outs[0].cpu().numpy(), raw["w.bf16"]) and np.array_equal(outs[2].cpu().numpy(), raw["ids.int64"])
        # check_base=False is the old call: OK, and bytes that are not the tensor
        outs, status = device_io.read_files_device(archive, planes="manifest", base=mixed, check_base=False)
        assert status == [OK] * 4 and not np.array_equal(outs[1].cpu().numpy(), raw["w.fp32"])
    # an archive without the field (the writers' default, and every archive from before it): the same entries under a manifest
    # without it read as they did, with any base
    plain_image = image.cpu().numpy().tobytes()
    old_manifest = json.dumps({"entries": list(old), "base_id": "step 0"}, separators=(",", ":")).encode()
    older = _with_manifest(plain_image, old_manifest)
    default = device_io.write_files_device(None, new, method=mc[0], level=mc[1], planes="dtype", base=old, base_id="step 0")
    e = zpk.parse(default)[-1]
    assert e["filename"] == device_io.DELTA_MANIFEST and default[e["offset"]:e["offset"] + e["comp_size"]] == old_manifest      # the writers' default: the manifest as it always was
    outs, status = device_io.read_files_device(older, planes="manifest", base=old, base_id="step 0")
    assert status == [OK] * len(new) and all(np.array_equal(got.cpu().numpy(), raw[name]) for name, got in zip(new, outs))
    outs, status = device_io.read_files_device(older, planes="manifest", base=mixed)
    assert status == [OK] * 4 and not np.array_equal(outs[1].cpu().numpy(), raw["w.fp32"])        # (nothing to check against: what it always did)
    # a malformed field raises like a malformed manifest
    bad = _with_manifest(plain_image, json.dumps({"entries": list(old), "base_id": "step 0", "base_xxh3": {k: "12" for k in old}}).encode())
    with pytest.raises(ValueError, match="delta.json does not parse"):
        device_io.read_files_device(bad, planes="manifest", base=old)


def _with_manifest(image, manifest):
    """the archive `image` with its last entry, DELTA_MANIFEST (stored), replaced by `manifest`: the payloads in front of it as they are"""
    ents = zpk.parse(image)
    last = ents[-1]
    assert last["filename"] == device_io.DELTA_MANIFEST and last["method"] == 0
    assert ents[0]["offset"] == 10 and all(a["offset"] + a["comp_size"] == b["offset"] for a, b in zip(ents, ents[1:]))      # back to back behind the data signature
    payloads = [image[e["offset"]:e["offset"] + e["comp_size"]] for e in ents[:-1]] + [manifest]
    table = [(e["filename"], e["offset"], e["comp_size"], e["uncomp_size"], e["hash"], e["method"]) for e in ents[:-1]]
    table.append((last["filename"], last["offset"], len(manifest), len(manifest), oracle().xxh3(manifest), 0))
    return zpk.assemble(payloads, table)


def test_hash_tensors_is_the_hash_field_of_the_same_tensors_written_as_plain_entries(torch, ckpt):
    tensors = dict(ckpt["new"], big=(torch.arange(300 * 1024 // 4 + 3, dtype=torch.int64, device="cuda:0") * 2654435761).to(torch.int32))     # 300 KiB + 12: chip-wide
    torch.cuda.synchronize()
    image = device_io.write_files_device(None, tensors, method=METHOD_LZ4, level=0)
    recorded = {e["filename"]: e["hash"] for e in zpk.parse(image)}
    got = device_io.hash_tensors(tensors)
    assert got == {k: recorded[k] for k in tensors}
    assert device_io.hash_tensors(list(tensors.values())) == [recorded[k] for k in tensors]
    sliced = tensors["w.fp32"][1:]                                                      # a view that starts 4 bytes into its allocation: its own bytes
    empty = torch.zeros(0, dtype=torch.float32, device="cuda:0")
    o = oracle()
    assert device_io.hash_tensors([sliced, empty]) == [o.xxh3(_bytes(sliced).tobytes()), o.xxh3(b"")]
    assert device_io.hash_tensors([]) == [] and device_io.hash_tensors({}) == {}
    with pytest.raises(ValueError):
        device_io.hash_tensors([torch.zeros(4)])                                        # host memory: not this call's
