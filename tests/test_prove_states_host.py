"""CPU suite: the per-item transcripts of bpp_prove_openings_device_transcripts as csrc/prove_ingest.h has them, on the host, lane by
lane, under AddressSanitizer + UBSan, held to ProvePack::pack and prove_item_check_host of the item form on the sorted equivalent
bpp_prove_item array in which every item has a transcript_state of its own.

The harness (csrc/hosttest_prove_states.cpp, a stand-alone program; nothing is preloaded) checks: the finding "transcript state has
pos >= rate" and its precedence (an item with a bad blinding factor, a bad nonce or a nonce at m > 1 beside a bad pos reports the
other finding); a bad pos alone at the first, a middle and the last item; pos = 165 (fine), 166 and 255; the plan's state_idx (the
slot's index in its sub-batch) and the size of d_states for 5, 17 and 67 items of the m pattern [1, 4, 2, 8, 1], with the sub-batch
cut at 64; the state rows the model of k_prove_item_states writes against the packer's advanced states, a failed slot under the fixed
public state; the out-row rule of the emit kernel -- give or zero, refused rows zeroed -- into rows at an odd address that end with
their allocation.  The bytes around the input rows are poisoned, and so is a bad row but for its byte 200 and a refused item's row as
a whole (whole granules of eight; in the first pass they hold 0xFF and nothing may depend on them)."""
import importlib
import os
import subprocess

CASES = ("plan_5_17_67", "bad_pos_first_middle_last", "pos_165_166_255", "precedence", "refused_rows", "every_row_bad")


def test_prove_item_states_equal_the_item_form_under_asan_ubsan():
    pkg = importlib.import_module("bulletproofs-plus_amd")
    exe = pkg._build.build_prove_states_harness()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    for case in CASES:
        assert "ok " + case in lines, (case, r.stdout[-2000:])
    assert "all ok" in lines and not any(line.startswith("FAIL") for line in lines)
    assert r.stderr.strip() == "", r.stderr[-4000:]
