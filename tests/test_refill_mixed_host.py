"""CPU suite: a refill of a batch of MIXED aggregation factors (bpp_batch_refill_enqueue_mixed) on the host, under AddressSanitizer +
UBSan.

The harness (csrc/hosttest_refill_mixed.cpp, a stand-alone program) holds the one-lane model of the refill kernels
(csrc/refill.h: refill_run_host<true>, plain, with a live count and under a live mask) to what a fresh device upload
(csrc/ingest.h, csrc/ingest_mixed.h: prelude, run, plan) makes of the rows in question -- all, the first c, the live ones alone in slot order: the
record (its index the slot of the upload's k-th row, the fall-back before a finding, a count beyond the batch before both), the live
slots byte for byte at the slots' own offsets, every dead or refused slot byte for byte the sanitised slot of ITS lengths, which
passes the walk of the upload.  The source arrays end behind the last live row; row slack and dead rows are poisoned, so a read of
either is an AddressSanitizer report, and a second run over full-length arrays with other strides leaves the same bytes.  Findings and
foreign first bytes lie at live and at dead slots, at the first and the last slot, in an m = 4 row and in a shortest row."""
import importlib
import os
import subprocess

CASES = ("clean_contents", "non_canonical_scalars", "nonce_on_aggregated_slots", "promises_above_the_capacity", "foreign_first_bytes",
         "several_findings", "a_slot_of_unfitting_length", "mutations", "uniform_rows_equal_packed")


def test_mixed_refill_equals_the_mixed_upload_of_the_live_rows_under_asan_ubsan():
    pkg = importlib.import_module("bulletproofs-plus_amd")
    exe = pkg._build.build_refill_mixed_harness()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    for case in CASES:
        assert "ok " + case in lines, (case, r.stdout[-2000:])
    assert "all ok" in lines and not any(line.startswith("FAIL") for line in lines)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
