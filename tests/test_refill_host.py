"""CPU suite: the one-lane host model of the kernels of bpp_batch_refill_enqueue (csrc/refill.h: refill_run_host) under
AddressSanitizer + UBSan, held to what a fresh device upload makes of the same arrays (csrc/ingest.h: ingest_run_host +
ingest_finish_plan, which tests/test_ingest_host.py holds to the host packer).

The harness (csrc/hosttest_refill.cpp, a stand-alone program) runs over the ingest harness's corpus -- the cases a resident batch can
meet -- extended by batches with two findings and with one foreign first byte, and asserts: a clean batch's bytes, promises, nonces,
flags and defer[] are the upload's; a batch with findings leaves the {code, message, index} the upload throws; an item with a finding
is not copied and its slot passes ingest_check_item, every other slot is the clean copy; a foreign first byte sets FALLBACK and claims
no finding; a second refill does not depend on the first; verdict_finish with a refill state gives the specified record and with a zero
state the existing routine."""
import importlib
import os
import subprocess

CASES = ("truncations_t1", "truncations_t3", "edge_scalars_t1", "edge_scalars_t3", "two_findings", "foreign_first_byte", "seed_with_m2",
         "nonces_m1", "promises_at_the_capacity", "degree_and_promise", "two_refills_in_a_row", "mutations",
         "verdict_finish_with_refill_state")


def test_refill_model_equals_the_device_upload_under_asan_ubsan():
    pkg = importlib.import_module("bulletproofs-plus_amd")
    exe = pkg._build.build_refill_harness()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    for case in CASES:
        assert "ok " + case in lines, (case, r.stdout[-2000:])
    assert "all ok" in lines and not any(line.startswith("FAIL") for line in lines)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
