"""CPU suite: the two concurrency protocols behind the verify / prove pipelines, the batcher and the prove pool
(csrc/lanes_host.h: tickets with worker lanes, and callers that lead pooled calls), driven by csrc/hosttest_lanes.cpp with integers
for lanes: once under ThreadSanitizer, once under AddressSanitizer + UBSan.  Stand-alone programs, run as child processes."""
import importlib
import os
import subprocess

import pytest

CASES = ("ticket_reverse_collect", "ticket_first_number", "ticket_dropped_claim", "ticket_run_throws", "ticket_unknown",
         "ticket_two_collectors", "ticket_done_states", "ticket_peek_then_refuse", "ticket_shutdown", "leader_groups_no_wait",
         "leader_groups_wait_200us", "leader_unpoolable_alone", "leader_woken_by_enqueue", "leader_run_throws", "leader_drain")


@pytest.mark.parametrize("kind", ["tsan", "asan"])
def test_lanes_under_sanitizers(kind):
    pkg = importlib.import_module("bulletproofs-plus_amd")
    exe = pkg._build.build_lanes_harness(kind)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=0:exitcode=66", ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    for case in CASES:
        assert "ok " + case in lines, (case, r.stdout[-2000:])
    assert "all ok" in lines
    assert r.stderr.strip() == "", r.stderr[-4000:]  # a sanitizer that has something to say says it here
