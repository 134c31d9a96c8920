"""CPU suite: the one-item routines of csrc/ingest.h in their mixed form with the host prelude and the plan of csrc/ingest_mixed.h -- what
bpp_batch_upload_mixed_device runs for a batch of mixed aggregation factors that lies in device memory -- on the host, under
AddressSanitizer + UBSan, held to the item form of csrc/upload_host.h on the equivalent bpp_verify_item array.

The harness (csrc/hosttest_ingest_mixed.cpp, a stand-alone program) runs them over a corpus and asserts for every case that {code,
message text, index} equal those of upload_pass_a + upload_pass_b, and on success that bytes[], promises, nonces, every ProofDesc
field, rounds_bad, defer and the plan's rmax / max_mn / total_dyn are equal.  Row slack is poisoned twice -- with values that would
change the outcome and with ASan's manual poisoning -- and every array ends with the last byte its last row uses.  The corpus: the
shapes of the GPU tests (1 / 5 / 17 / 67 items of the m pattern); every length of a proof at index 3 of 7 between valid items of other
m; non-canonical scalars; 64 and 65 (L, R) pairs; first byte 0 and 7; a nonce on an m = 2 item; host-known findings (m = 3, 0, 8) with
a device finding below and above them; null arrays; the geometry refusals and the size limit; promises at the capacity per entry of an
m = 4 item; a transcript state with pos >= rate; mixed first bytes; random mutations."""
import importlib
import os
import subprocess

CASES = ("valid_shapes", "one_item", "lengths_at_index_3", "length_findings", "non_canonical_scalars", "wire_rounds_64_and_65",
         "first_byte_0_and_7", "nonce_on_an_m2_item", "host_known_findings", "null_arrays", "geometry_refusals", "size_limit",
         "promises_at_the_capacity", "degree_and_promise", "rounds_bad", "bad_transcript_state", "mixed_first_bytes_fall_back", "mutations",
         "uniform_rows_equal_packed")


def test_mixed_ingest_equals_the_item_form_under_asan_ubsan():
    pkg = importlib.import_module("bulletproofs-plus_amd")
    exe = pkg._build.build_ingest_mixed_harness()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    for case in CASES:
        assert "ok " + case in lines, (case, r.stdout[-2000:])
    assert "all ok" in lines and not any(line.startswith("FAIL") for line in lines)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
