"""CPU suite: a refill under a per-item live mask (bpp_batch_refill_enqueue_live) on the host, under AddressSanitizer + UBSan.

The harness (csrc/hosttest_refill_live.cpp, a stand-alone program) holds the one-lane model of the refill kernels (csrc/refill.h:
refill_run_host with a mask) to what a fresh device upload makes of the LIVE ITEMS ALONE, in slot order (csrc/ingest.h), under the
masks all dead, all live, one live item at 0 / N - 1, alternating, a dead run in the middle and the byte values 2 and 255, with
findings and foreign first bytes at live and at dead items: the record (its index the slot of the upload's k-th item), the live slots
byte for byte, every dead slot byte for byte the sanitised slot, the batch's mask normalised, the count word untouched.  The sources
of dead items are never read: the arrays the model is handed end behind the last live item and hold a poison pattern at every dead
item, and a second run over full-length arrays leaves the same bytes, none of them the pattern.  It then holds the live routines of
csrc/verdict.h over a mask plus verdict_finish to check_deferred + check_chunk_errors on the compacted groups, an empty group between
two live ones among them, with the reference's index mapped to the slot offset."""
import importlib
import os
import subprocess

CASES = ("edge_scalars_t1", "edge_scalars_t3", "truncations_t1", "two_findings", "foreign_first_byte", "nonces", "promises_and_degree",
         "mutations", "compacted_groups")


def test_refill_under_a_mask_equals_the_upload_of_the_live_items_under_asan_ubsan():
    pkg = importlib.import_module("bulletproofs-plus_amd")
    exe = pkg._build.build_refill_live_harness()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    for case in CASES:
        assert "ok " + case in lines, (case, r.stdout[-2000:])
    assert "all ok" in lines and not any(line.startswith("FAIL") for line in lines)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
