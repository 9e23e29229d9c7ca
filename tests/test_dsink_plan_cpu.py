"""CPU: a batch compressed into a bounded sink in device memory, as zpack_amd/csrc/dsink_plan.h decides it for
zpk_codec_encode_batch_dsink and for the kernels k_sink_cut / k_sink_place (the harness compiles the very header they include) under
AddressSanitizer + UBSan: the cut under the reference's append rule, the span table and what the persistent grid copies from it, room
and chaining of sub-batches, the staging slots (tools/hostfuzz/dsink_plan_main.cpp).  A model of the cut written here agrees with the
driver's answers on a fixed list of statuses, sizes and rooms."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "tools", "hostfuzz", "run_dsink_plan.sh")

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with the sanitizer runtimes")


def model_cut(batch, room):
    """the append rule of lib/zpack_write.c:299-303 with "does not fit" as one more failure: the files in front of the first that
    failed or would end behind the room -> (placed, bytes)"""
    placed = nbytes = 0
    for status, size in batch:
        if status != 0 or nbytes + size > room:
            break
        placed += 1
        nbytes += size
    return placed, nbytes


@needs_gxx
def test_dsink_plan_under_asan_ubsan():
    p = subprocess.run(["bash", RUN], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    for line in ("cut: 32876:5/32876 32875:4/32869 0:0/0 100:2/100 99:0/0 16484:3/16484 16483:2/100 1048576:5/32876",
                 "failed: at 0 0/0, at the last 2/11, at the last with room for one 1/5, in the middle 1/9, behind a file that does not fit 0/0",
                 "wrap: two sizes whose sum passes 2^64 stop at the second, whatever the room",
                 "spans: sizes 0, 1, 16384, 16385 are 0, 1, 1, 2 items; a ragged batch of one 256 MiB entry and 30000 of 100 bytes is 46384 items in 11596 slots and a grid of 2048",
                 "chain: sub-batches of 5, 3 and 4 entries of which the last places 1 end the call at 9 entries and 1017 bytes",
                 "random: 3000 batches at 8 rooms each,"):
        assert line in p.stdout, p.stdout[-1500:]
    # the fixed lines are what the model says too
    ok = [(0, 100), (0, 0), (0, 16384), (0, 16385), (0, 7)]
    want = " ".join("%d:%d/%d" % ((room,) + model_cut(ok, room)) for room in (32876, 32875, 0, 100, 99, 16484, 16483, 1 << 20))
    assert "cut: " + want in p.stdout


OK5 = [(0, 100), (0, 0), (0, 16384), (0, 16385), (0, 7)]                              # 32876 bytes
CASES = [
    (OK5, 32876),                                 # room exactly equal to the batch
    (OK5, 32875),                                 # one byte short
    (OK5, 0),                                     # zero room: the entry without bytes behind entry 0 does not get in either
    ([(0, 0), (0, 0), (0, 5)], 0),                # zero room takes the entries without bytes in front
    ([(14, 0), (0, 5), (0, 6)], 1000),            # a failure at index 0
    ([(0, 5), (0, 6), (12, 0)], 1000),            # a failure at the last index
    ([(0, 5), (0, 6), (12, 0)], 10),              # ... behind a file that does not fit
    ([(0, 9), (19, 0), (0, 9), (0, 9)], 1000),    # a failure in the middle stops the files behind it
    ([(0, 16384)] * 4, 3 * 16384),                # whole spans, room for three
    ([(0, 16385)] * 4, 3 * 16385 + 16384),        # one byte into the next span short
    ([], 0),
    ([(0, 1 << 40), (0, 1)], (1 << 40) + 1),
]


@needs_gxx
@pytest.mark.parametrize("case", range(len(CASES)))
def test_the_model_of_the_cut_agrees_with_the_driver(case):
    batch, room = CASES[case]
    p = subprocess.run(["bash", RUN, "cut", str(room)] + ["%d:%d" % e for e in batch], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    placed, nbytes = (int(x) for x in p.stdout.split())
    assert (placed, nbytes) == model_cut(batch, room)


def test_the_model_on_the_named_cases():
    assert model_cut(OK5, 32876) == (5, 32876) and model_cut(OK5, 32875) == (4, 32869) and model_cut(OK5, 0) == (0, 0)
    assert model_cut(CASES[4][0], 1000) == (0, 0) and model_cut(CASES[5][0], 1000) == (2, 11) and model_cut(CASES[3][0], 0) == (2, 0)
