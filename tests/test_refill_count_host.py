"""CPU suite: a refill with a live count (bpp_batch_refill_enqueue_count) on the host, under AddressSanitizer + UBSan.

The harness (csrc/hosttest_refill_count.cpp, a stand-alone program) holds the one-lane model of the refill kernels (csrc/refill.h:
refill_run_host with a count) to what a fresh device upload makes of the FIRST c ITEMS of the same arrays (csrc/ingest.h), for
c in {0, 1, N - 1, N, N + 1}, with findings and foreign first bytes on both sides of c: the record, the live slots, every dead slot
byte for byte the sanitised slot, the batch's live word.  The sources of dead items are never read: the arrays the model is handed
end behind the last live item, and a second run over arrays whose dead items hold a poison pattern leaves the same bytes, none of
them the pattern.  It then holds the two live routines of csrc/verdict.h plus verdict_finish to check_deferred + check_chunk_errors
on the cut batch, for groups cut in the middle, exactly at a boundary, and empty."""
import importlib
import os
import subprocess

CASES = ("edge_scalars_t1", "edge_scalars_t3", "truncations_t1", "two_findings", "foreign_first_byte", "nonces", "promises_and_degree",
         "mutations", "cut_groups")


def test_refill_with_a_count_equals_the_upload_of_the_first_items_under_asan_ubsan():
    pkg = importlib.import_module("bulletproofs-plus_amd")
    exe = pkg._build.build_refill_count_harness()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    for case in CASES:
        assert "ok " + case in lines, (case, r.stdout[-2000:])
    assert "all ok" in lines and not any(line.startswith("FAIL") for line in lines)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
