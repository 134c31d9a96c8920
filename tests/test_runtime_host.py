"""CPU suite: the host runtime around the engine's calls (csrc/runtime_host.h: the small-call gate, the persistent worker pool, the
nap schedule of a waiting caller) and the chain scheduler (csrc/chain_host.h), driven by csrc/hosttest_runtime.cpp without a GPU:
once under ThreadSanitizer, once under AddressSanitizer + UBSan.  Stand-alone programs, run as child processes."""
import importlib
import os
import subprocess

import pytest

CASES = ("gate_fifo_under_limit", "gate_reentrant", "gate_off", "gate_large_passes", "gate_widen_and_remove", "env_long",
         "pool_size_from_env", "pool_covers_once", "pool_idle_not_busy", "pool_cpu_ns_counts", "cpus_from_quota",
         "chain_width_rule", "chain_units_ragged", "chains_lockstep_equals_scalar",
         "wait_cold", "wait_remembered", "wait_late_first_look", "wait_floor", "wait_tail_spin", "wait_hint_fold", "nap_timespec")


@pytest.mark.parametrize("kind", ["tsan", "asan"])
def test_runtime_under_sanitizers(kind):
    pkg = importlib.import_module("bulletproofs-plus_amd")
    exe = pkg._build.build_runtime_harness(kind)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=0:exitcode=66", ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    for case in CASES:
        assert "ok " + case in lines, (case, r.stdout[-2000:])
    assert "all ok" in lines
    assert r.stderr.strip() == "", r.stderr[-4000:]  # a sanitizer that has something to say says it here
