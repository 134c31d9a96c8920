"""CPU suite: the verdict resolution of csrc/verdict.h -- what k_verdict_scan and k_verdict_finish run behind the final MSM of
bpp_verify_enqueue -- on the host, under AddressSanitizer + UBSan, held to the host rules of the blocking calls.

The harness (csrc/hosttest_verdict.cpp, a stand-alone program) asserts that verdict_key + minimum + verdict_finish + verdict_message
give the code, tier, index and message text of check_deferred + check_chunk_errors (csrc/upload_host.h) plus the final-check line of
verify_flow_once: exhaustively for groups of 1-3 proofs over every (status 0..7, rounds_bad in {0, InvalidLength, SizeOverflow},
defer 0..3) per proof x identity flag x three actions x zero-weight flag, and for 10 000 seeded random groups of up to 600 proofs
with sparse findings.  A redraw (zero weight in a group that needed weights) must claim nothing else."""
import importlib
import os
import subprocess

CASES = ("exhaustive_1", "exhaustive_2", "exhaustive_3", "random_groups", "texts")


def test_shared_verdict_resolution_equals_the_host_rules_under_asan_ubsan():
    pkg = importlib.import_module("bulletproofs-plus_amd")
    exe = pkg._build.build_verdict_harness()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    for case in CASES:
        assert "ok " + case in lines, (case, r.stdout[-2000:])
    assert "all ok" in lines and not any(line.startswith("FAIL") for line in lines)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
