"""CPU: the side tables of the host library — the records libzpack_amd.so keeps beside zpack_reader and zpack_writer structs, keyed by
their addresses (zpack_amd/host/util.c: zi_side_find / _set / _drop) — under a stand-alone driver that is linked with the very util.c the
library compiles (tools/hostfuzz/side_table_main.c), built and run once under AddressSanitizer + UBSan and once under ThreadSanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "tools", "hostfuzz", "run_side_table.sh")

LINES = ("empty: nothing found, the caller's record untouched",
         "set: found with its three fields",
         "replace: a second set at the key replaced the record, one drop forgot it",
         "chain: 1000 keys in one bucket, 6 dropped from the middle, the head and the tail, 994 found and dropped after",
         "missing: dropping a key that is not there changes nothing",
         "instances: one key in two tables, two records, dropped one by one",
         "threads: 8 finders and 2 writers, 10000 operations each, 0 torn or missing records",
         "ok")


def test_side_table_under_asan_ubsan_and_tsan():
    p = subprocess.run(["bash", RUN], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    runs = p.stdout.split("== -fsanitize=")
    assert [r.split("\n", 1)[0] for r in runs[1:]] == ["address,undefined", "thread"], p.stdout[-1500:]
    for run in runs[1:]:
        assert run.split("\n")[1:len(LINES) + 1] == list(LINES), run
    assert "FAILED" not in p.stdout and "Sanitizer" not in p.stderr, p.stderr[-2000:]
