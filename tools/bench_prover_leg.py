#!/usr/bin/env python3
"""The prover leg of bench.py alone (configs[4]: 1024 x aggregation-4, extension degree 3): proofs/s one call at a time over 8
calls, k_fb_msm's summed event time and rate per call.  One line.

  --check            every proof verified before it is returned (the context's "prove_check" = 1); the line adds the check's counters
  --check-recovery   with --check: mask recovery replayed for the proofs that carry a seed nonce ("prove_check_recovery" = 1)
  --nonces           instead of configs[4]: 1024 proofs of n = 64, m = 1, extension degree --t (default 3), a seeded nonce on each
                     (an aggregated statement cannot carry one)
  --openings         prove from the openings alone: ONE bpp_prove_openings call per step, the commitments made by the engine
  --openings-two-call  the same output the way it took two calls: bpp_pedersen_commit, then bpp_prove_batch over what it returned,
                     timed together"""
import argparse
import importlib
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help='"prove_check" = 1 on the context')
    ap.add_argument("--check-recovery", action="store_true", help='"prove_check_recovery" = 1 on the context')
    ap.add_argument("--nonces", action="store_true", help="1024 x (n = 64, m = 1) with a seed nonce each instead of configs[4]")
    ap.add_argument("--openings", action="store_true", help="one bpp_prove_openings call: commitments made by the engine")
    ap.add_argument("--openings-two-call", action="store_true", help="bpp_pedersen_commit + bpp_prove_batch, timed together")
    ap.add_argument("--t", type=int, default=3, help="extension degree of the --nonces proofs")
    args = ap.parse_args()
    import numpy as np
    import bench
    bpp = importlib.import_module("bulletproofs-plus_amd")
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    eng = bpp.Engine(0)
    eng.profile(True)
    if args.check:
        eng.set_option("prove_check", 1)
    if args.check_recovery:
        eng.set_option("prove_check_recovery", 1)
    if args.nonces:
        p5 = bpp.RangeParameters.init(64, 1, bpp.create_pedersen_gens_with_extension_degree(args.t), engine=eng)
    else:
        p5 = bpp.RangeParameters.init(64, 4, bpp.create_pedersen_gens_with_extension_degree(3), engine=eng)
    d5 = bench.make_inputs(np, packed, p5, 1024, seed=8675309 + 5)  # (seed nonces iff m = 1)
    iters = int(os.environ.get("PROVER_ITERS", "8"))

    def step():
        if args.openings:
            return packed.prove(p5, d5["values"], d5["blindings"], None, d5["min_values"], d5["min_present"], d5["seeds"], bench.LABEL, d5["ext"])[1]
        comm = d5["commitments"]
        if args.openings_two_call:
            n, m = d5["values"].shape
            comm = packed.commit(p5, d5["values"].reshape(n * m), d5["blindings"].reshape(n * m, -1, 32)).reshape(n, m, 32)
        return packed.prove(p5, d5["values"], d5["blindings"], comm, d5["min_values"], d5["min_present"], d5["seeds"], bench.LABEL, d5["ext"])

    for _ in range(2):
        step()
    t0 = time.perf_counter()
    for _ in range(iters):
        out = step()
    el = time.perf_counter() - t0
    assert out.shape[0] == 1024
    pp = eng.last_prove_profile()
    rec = {"proofs_per_s": round(1024 * iters / el), "ms_per_call": round(1e3 * el / iters, 3), "fb_msm_ms": round(pp["fb_msm_ms"], 3),
           "fb_G_adds_per_s": round(pp["fb_terms"] * pp["fb_windows"] / (pp["fb_msm_ms"] * 1e-3) / 1e9, 2), "engine_total_ms": round(pp["total_ms"], 3)}
    if args.check:
        rec["check"] = eng.prove_check_stats()
    if args.check_recovery:
        rec["check_recovery"] = eng.prove_check_recovery_stats()
    if args.nonces:
        rec.update(nonces=1, extension_degree=args.t)
    if args.openings or args.openings_two_call:
        rec.update(form="openings" if args.openings else "openings-two-call")
    print(json.dumps(rec))
    p5.close()
    eng.close()


if __name__ == "__main__":
    main()
