"""CPU suite: csrc/prove_ingest.h as bpp_prove_enqueue uses it, on the host under AddressSanitizer + UBSan.

The harness (csrc/hosttest_prove_enqueue.cpp, a stand-alone program; nothing is preloaded) runs
  - the ingest routines (and the model of k_prove_item_states) under live masks -- all live, all dead, alternating, only the first, only
    the last -- on 1, 5 and 67 items of the m pattern [1, 4, 2, 8, 1] at t = 1 and 3, with one transcript for the call and with one row
    per item, commitments brought and made, 16 lanes per item and one.  Live slots must equal ProvePack::pack on the equivalent items,
    dead slots the substitute witness and the fixed public state, with BPP_PROVE_MSG_EMPTY in their finding word.  Every array ends
    behind the last live row; the rows of dead items hold 0xFF (each a finding if it were read) in one pass and are poisoned in the
    other, so that a read of a dead row is an ASan report;
  - the emit routine's ok mask and outcome table and the summary reduction (256 lanes and one) against a plain host loop, over tables
    of 1, 5, 67 and 700 items with a finding at the first, a middle and the last index, two findings, none, refused items interleaved
    with failed and dead ones, all empty, all failed."""
import importlib
import os
import subprocess

MASKS = ("all_live", "all_dead", "alternating", "only_first", "only_last")


def test_live_mask_and_summary_under_asan_ubsan():
    pkg = importlib.import_module("bulletproofs-plus_amd")
    exe = pkg._build.build_prove_enqueue_harness()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    for mask in MASKS:
        assert "ok live_mask_" + mask in lines, (mask, r.stdout[-2000:])
    for n in (1, 5, 67, 700):
        wanted = ["summary_none", "summary_finding_at_0", "summary_finding_at_%d" % (n // 2), "summary_finding_at_%d" % (n - 1),
                  "summary_all_empty", "summary_all_fail"]
        if n >= 5:
            wanted += ["summary_two_findings", "summary_refused_interleaved"]
        for case in wanted:
            assert "ok %s_%d" % (case, n) in lines, (case, n, r.stdout[-2000:])
    assert "all ok" in lines and not any(line.startswith("FAIL") for line in lines)
    assert r.stderr.strip() == "", r.stderr[-4000:]
