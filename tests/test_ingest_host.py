"""CPU suite: the one-item routines of csrc/ingest.h -- what the kernel of bpp_batch_upload_packed_device runs per proof of a packed
batch that lies in device memory -- on the host, under AddressSanitizer + UBSan, held to the host packer of csrc/upload_host.h.

The harness (csrc/hosttest_ingest.cpp, a stand-alone program) runs them over a corpus and asserts for every case that {code, message
text, index} equal those of upload_pass_a_packed + upload_pass_b_packed (or of the item form where pass A declines), and on success
that descriptors (flags included), promises, nonces, staged bytes, rounds_bad and defer are equal.  The corpus: every truncation of a
valid t = 1 and t = 3 proof (also under a non-canonical d1[0]: it beats a body too short for r1); first byte 0 and 7; l, l - 1, 2^255
and all ones in each of d1[k], r1, s1, alone and in pairs; 64 and 65 (L, R) pairs; a seed nonce with m = 2; a transcript state with
pos >= rate at item 0, behind a good and behind a bad proof; promises 2^n - 1 and 2^n at n = 8; what is uniform over the batch; mixed
first bytes; random mutations."""
import importlib
import os
import subprocess

CASES = ("truncations_t1", "truncations_t3", "first_byte_0_and_7", "edge_scalars_t1", "edge_scalars_t3", "wire_rounds_64_and_65",
         "seed_with_m2", "nonces_m1", "bad_transcript_state", "promises_at_the_capacity", "promise_of_an_aggregated_item",
         "degree_and_promise", "rounds_bad", "uniform_findings", "size_limit", "mixed_first_bytes_fall_back", "mutations")


def test_one_item_ingest_equals_the_host_packer_under_asan_ubsan():
    pkg = importlib.import_module("bulletproofs-plus_amd")
    exe = pkg._build.build_ingest_harness()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    for case in CASES:
        assert "ok " + case in lines, (case, r.stdout[-2000:])
    assert "all ok" in lines and not any(line.startswith("FAIL") for line in lines)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
