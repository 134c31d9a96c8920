#!/usr/bin/env python3
"""The transcript RNG on the stream (bpp_transcripts_enqueue with the RNG kinds) against the host route, in one process on an engine
made on torch's stream; and the existing NEW + APPEND + CHALLENGE program on this tree against the parent commit's library.

Part 1, at n = 1024 and 65 536 rows, the program that makes a prover's randomness from a secret row and 32 bytes of entropy per item:
  RNG_BEGIN, RNG_REKEY("witness", 32 B), RNG_FINALIZE(entropy), RNG_FILL32 of a configs[4]-shaped rng row ((8 + 3) x 32 = 352 bytes:
  64 bits, aggregation factor 4), RNG_SCALARS x m (m = 4)
  device arm: K calls on the stream, one stream synchronise, wall time / K (K grows until the window is --window seconds)
  host arm:   the same bytes made with the host helpers (bpp_transcript_rng_begin / _rekey / _finalize / _fill x 11 / _scalar x 4 per
              row) on one core, plus the copy of the rng rows and the blinding factors to the device.  From Python every helper call
              goes through ctypes; `ctypes_overhead_ms` is the measured cost of as many empty ctypes calls, `host_ms_less_ctypes` what a
              compiled caller would see.
Part 2 (--existing-only): the NEW + APPEND(32 B) + CHALLENGE(32) program alone, ms per call at the same sizes, one JSON line.  That is
  the command of an alternating A/B against the parent commit's library (a program of these kinds runs the kernel it always ran):
    tools/gpu_ab.py --leg cmd --cmd "python tools/bench_transcript_rng.py --existing-only" --reps 3 --out rng_ab.txt \
        "BPP_LIB_PATH=<the parent commit's libbpp_hip.so>" "" "BPP_LIB_PATH=<the same>"
  The parent arm stands twice in every repetition: the differences among its own runs are the run-to-run spread this tree's figure is
  held to.  --merge-ab FILE reads the runner's lines into the record ("existing_program_ab").
No figure is asserted: a record, not a gate.  Prints one JSON line; the record goes to --out (profiles/transcript_rng.json)."""
import argparse
import ctypes
import importlib
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RNG_ROW, M = 32 * (8 + 3), 4  # configs[4]: 64 bits x aggregation factor 4 -> 8 rounds, rounds + 3 draws of 32 bytes


def merge_ab(path, out):
    """tools/gpu_ab.py's lines ("rep=N [arm] {json}") -> {"parent": {size: [ms per call]}, "this": {...}} into the record"""
    arms = {"parent": {}, "this": {}}
    for line in open(path):
        m = re.match(r"rep=\d+ \[(.*?)\] (\{.*\})\s*$", line)
        if not m:
            continue
        arm = "parent" if "BPP_LIB_PATH" in m.group(1) else "this"
        for size, ms in json.loads(m.group(2))["existing_program_ms_per_call"].items():
            arms[arm].setdefault(size, []).append(ms)
    doc = json.load(open(out)) if os.path.exists(out) else {"tool": "bench_transcript_rng"}
    ab = {"program": "NEW + APPEND(32 B) + CHALLENGE(32)", "unit": "ms per call", "sizes": {}}
    for size in sorted(arms["parent"], key=int):
        p, t = arms["parent"][size], arms["this"].get(size, [])
        ab["sizes"][size] = {"parent": p, "this": t, "parent_median": statistics.median(p), "this_median": statistics.median(t) if t else None,
                             "parent_spread": [min(p), max(p)], "this_inside_parent_spread": bool(t) and statistics.median(t) <= max(p)}
    doc["existing_program_ab"] = ab
    json.dump(doc, open(out, "w"), indent=1)
    print(json.dumps({"tool": "bench_transcript_rng", "existing_program_ab": ab["sizes"]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,65536")
    ap.add_argument("--window", type=float, default=1.0, help="seconds of device calls per timed window")
    ap.add_argument("--host-steps", type=int, default=2)
    ap.add_argument("--existing-only", action="store_true", help="part 2: the NEW + APPEND + CHALLENGE program alone, one line, no record")
    ap.add_argument("--merge-ab", default=None, help="a file of tools/gpu_ab.py lines of --existing-only runs: merged into the record")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transcript_rng.json"))
    args = ap.parse_args()
    if args.merge_ab:
        return merge_ab(args.merge_ab, args.out)
    import numpy as np
    import torch
    bpp = importlib.import_module("bulletproofs-plus_amd")
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    stream = torch.cuda.Stream()
    sizes = [int(x) for x in args.sizes.split(",")]
    rec = {"tool": "bench_transcript_rng", "box": torch.cuda.get_device_name(0), "window_s": args.window, "rng_row_bytes": RNG_ROW, "scalars": M,
           "sizes": []}
    l_wit = b"witness"
    c_wit = (ctypes.c_uint8 * len(l_wit)).from_buffer_copy(l_wit)
    with torch.cuda.stream(stream):
        eng = bpp.Engine(0, stream=stream.cuda_stream)
        lib = eng.lib

        def window(fn):
            k = 8
            while True:
                stream.synchronize()
                t0 = time.perf_counter()
                for _ in range(k):
                    fn()
                stream.synchronize()
                dt = time.perf_counter() - t0
                if dt >= args.window or k >= (1 << 17):
                    return dt / k * 1e3, k
                k = min(k * max(2, int(args.window / max(dt, 1e-4)) + 1), 1 << 17)

        existing = {}
        for n in sizes:
            rng = np.random.default_rng(n)
            done, record = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
            txid = torch.from_numpy(rng.integers(0, 256, size=(n, 32), dtype=np.uint8)).cuda()
            rows = torch.full((n, 203), 0xFF, dtype=torch.uint8, device="cuda")
            chal = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
            old_ops = [packed.TNew(b"bench transcript rng"), packed.TAppend(b"txid", txid), packed.TChallenge(b"next", 32, chal)]
            old = lambda: packed.transcript_ops(eng, rows, old_ops, done_mask=done, record=record)  # noqa: E731
            old().wait()
            assert int(record.cpu()[0]) == n
            old(), old()
            existing[str(n)] = window(old)[0]
            if args.existing_only:
                continue
            secret = torch.from_numpy(rng.integers(0, 256, size=(n, 32), dtype=np.uint8)).cuda()
            entropy = torch.from_numpy(rng.integers(0, 256, size=(n, 32), dtype=np.uint8)).cuda()
            ext = torch.zeros((n, RNG_ROW), dtype=torch.uint8, device="cuda")
            blind = torch.zeros((n, 32 * M), dtype=torch.uint8, device="cuda")
            ext_host, blind_host = torch.zeros_like(ext), torch.zeros_like(blind)
            ops = [packed.TRngBegin(), packed.TRngRekey(l_wit, secret), packed.TRngFinalize(entropy), packed.TRngFill32(RNG_ROW, ext),
                   packed.TRngScalars(M, blind)]
            dev_fn = lambda: packed.transcript_ops(eng, rows, ops, done_mask=done, record=record)  # noqa: E731
            rows_np, secret_np, entropy_np = rows.cpu().numpy(), secret.cpu().numpy(), entropy.cpu().numpy()

            def host_fn():
                """the host route: the helpers per row on one core, then the rng rows and the blinding factors up"""
                e, b = np.zeros((n, RNG_ROW), dtype=np.uint8), np.zeros((n, 32 * M), dtype=np.uint8)
                st = (ctypes.c_uint8 * 203)()
                rb, sb, nb, eb, bb = rows_np.ctypes.data, secret_np.ctypes.data, entropy_np.ctypes.data, e.ctypes.data, b.ctypes.data
                for i in range(n):
                    lib.bpp_transcript_rng_begin(rb + 203 * i, st)
                    lib.bpp_transcript_rng_rekey(st, c_wit, len(l_wit), sb + 32 * i, 32)
                    lib.bpp_transcript_rng_finalize(st, nb + 32 * i)
                    for k in range(RNG_ROW // 32):
                        lib.bpp_transcript_rng_fill(st, eb + RNG_ROW * i + 32 * k, 32)
                    for k in range(M):
                        lib.bpp_transcript_rng_scalar(st, bb + 32 * M * i + 32 * k, None, 0)
                ext_host.copy_(torch.from_numpy(e))
                blind_host.copy_(torch.from_numpy(b))
                torch.cuda.current_stream().synchronize()

            def ctypes_overhead(calls):
                best = None
                for _ in range(3):
                    t0 = time.perf_counter()
                    for _ in range(calls):
                        lib.bpp_host_threads()
                    dt = (time.perf_counter() - t0) * 1e3
                    best = dt if best is None else min(best, dt)
                return best

            # what is timed is right: both routes give the same bytes
            dev_fn().wait()
            host_fn()
            assert torch.equal(ext, ext_host) and torch.equal(blind, blind_host), "the device differs from the host route"
            dev_fn(), dev_fn()
            dev_ms, k = window(dev_fn)
            hs = []
            for _ in range(args.host_steps if n > 4096 else 4 * args.host_steps):
                t0 = time.perf_counter()
                host_fn()
                hs.append((time.perf_counter() - t0) * 1e3)
            host_ms, over = statistics.median(hs), ctypes_overhead((3 + RNG_ROW // 32 + M) * n)
            rec["sizes"].append({"n": n, "device_ms_per_call": dev_ms, "device_calls_in_window": k, "device_rows_per_s": n / dev_ms * 1e3,
                                 "host_ms_per_step": host_ms, "host_ms_low": min(hs), "host_ms_high": max(hs), "ctypes_overhead_ms": over,
                                 "host_ms_less_ctypes": host_ms - over, "host_over_device": host_ms / dev_ms,
                                 "host_less_ctypes_over_device": (host_ms - over) / dev_ms, "existing_program_ms_per_call": existing[str(n)]})
        stats = packed.transcripts_stats(eng)
        eng.close()
    if args.existing_only:
        print(json.dumps({"tool": "bench_transcript_rng", "existing_program_ms_per_call": existing}))
        return
    rec["stats"] = stats
    old = json.load(open(args.out)) if os.path.exists(args.out) else {}
    if "existing_program_ab" in old:
        rec["existing_program_ab"] = old["existing_program_ab"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
    print(json.dumps({"tool": "bench_transcript_rng", "device_ms_per_call": {str(r["n"]): round(r["device_ms_per_call"], 4) for r in rec["sizes"]},
                      "host_over_device": {str(r["n"]): round(r["host_over_device"], 1) for r in rec["sizes"]},
                      "existing_program_ms_per_call": {k: round(v, 4) for k, v in existing.items()}}))


if __name__ == "__main__":
    main()
