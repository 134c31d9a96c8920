"""CPU suite: per-item transcripts on the device paths (csrc/item_states.h) on the host, under AddressSanitizer + UBSan.

The harness (csrc/hosttest_item_states.cpp, a stand-alone program) holds the one-lane model of k_item_states -- every row, under a
live count, under a live mask -- to what upload_host.h makes of the equivalent item array, the live items in slot order with
transcript_state = the row of their slot: the states table (through state_idx), tr_err_index, and code, text and index of what the
item form throws.  Bad states (pos 166 and 255) lie at live and dead slots, at the first and the last slot, alone, and together with a
non-canonical scalar at the same, a lower and a higher index.  Dead rows are poisoned and the source ends behind the last live row
(an exact-size allocation: a load from a dead row behind it is an AddressSanitizer report); the source starts at each of the four
byte offsets.  The row rule of k_states_out is held to a table of records and liveness views, the caller's array at each offset."""
import importlib
import os
import subprocess

FORMS = (0, 1, 2)
CASES = ("clean", "bad first", "bad last", "two bad, the lower wins", "bad scalar at the same index wins",
         "bad scalar at a higher index loses", "bad scalar at a lower index wins")
PARTIAL_CASES = ("bad states at dead slots only", "bad states at dead slots and the last live one")
OTHERS = ("item_states one item, clean", "item_states one item, bad", "item_states count 0", "item_states mask of zeros",
          "item_states count beyond the batch", "item_states n_run")


def test_item_states_model_equals_the_item_form_under_asan_ubsan():
    pkg = importlib.import_module("bulletproofs-plus_amd")
    exe = pkg._build.build_item_states_harness()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    for form in FORMS:
        for off in range(4):
            for case in CASES + (PARTIAL_CASES if form else ()):
                assert "ok item_states form=%d offset=%d %s" % (form, off, case) in lines, (form, off, case, r.stdout[-2000:])
    for case in OTHERS:
        assert "ok " + case in lines, (case, r.stdout[-2000:])
    assert any(line.startswith("ok states_out ") for line in lines), r.stdout[-2000:]
    assert "all ok" in lines and not any(line.startswith("FAIL") for line in lines)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
