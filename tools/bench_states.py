#!/usr/bin/env python3
"""What asking for the advanced transcripts costs (include/bpp.h, "Advanced transcripts"): one call at a time, the same call with
and without the state buffer.  One JSON line; made for `tools/gpu_ab.py --leg cmd`, one arm per setting:

  tools/gpu_ab.py --leg cmd --cmd "python tools/bench_states.py --what verify" --reps 3 "--states 0" "--states 1"
  tools/gpu_ab.py --leg cmd --cmd "python tools/bench_states.py --what prove" --reps 3 "--states 0" "--states 1"

  --what verify   a resident batch of --n (1024) non-aggregated 64-bit proofs, VerifyOnly, chunk 0: bpp_verify_resident against
                  bpp_verify_resident_states; --wave 0 / 1 forces the one-lane / one-wavefront form of PASS 1 (-1: the engine's rule)
  --what prove    configs[4] of the benchmark (1024 x aggregation 4, extension degree 3): bpp_prove_batch_mixed against
                  bpp_prove_batch_mixed_states"""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys
import time
from ctypes import POINTER, c_size_t

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def verify(args, bpp):
    from tests.golden.loader import load_bench
    data = load_bench("bench_cfg2.bin")
    eng = bpp.Engine(0)
    eng.set_option("transcripts_wave", args.wave)
    params = bpp.RangeParameters.init(data["bit_length"], data["m"], bpp.create_pedersen_gens_with_extension_degree(data["t"]), engine=eng)
    its = (data["items"] * ((args.n + len(data["items"]) - 1) // len(data["items"])))[:args.n]
    sts = [bpp.RangeStatement.init(params, it["commitments"], it["min_values"], None) for it in its]
    rb = bpp.ResidentBatch([bpp.Transcript.new(data["label"]) for _ in its], sts, [bpp.RangeProof.from_bytes(it["proof"]) for it in its])
    err = ctypes.create_string_buffer(256)
    buf = (ctypes.c_uint8 * (203 * args.n))()

    def call():
        if args.states:
            rc = eng.lib.bpp_verify_resident_states(eng.ctx, rb.handle, 0, 0, None, None, buf, err, 256)
        else:
            rc = eng.lib.bpp_verify_resident(eng.ctx, rb.handle, 0, 0, None, None, err, 256)
        assert rc == 0, err.value
    for _ in range(20):
        call()
    lat = []
    for _ in range(args.iters):
        t0 = time.perf_counter()
        call()
        lat.append(time.perf_counter() - t0)
    rb.close()
    params.close()
    eng.close()
    return {"what": "verify", "n": args.n, "wave": args.wave, "states": args.states, "ms_median": round(1e3 * statistics.median(lat), 4),
            "ms_min": round(1e3 * min(lat), 4)}


def prove(args, bpp):
    import numpy as np
    import bench
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    _lib = bpp._lib
    eng = bpp.Engine(0)
    p5 = bpp.RangeParameters.init(64, 4, bpp.create_pedersen_gens_with_extension_degree(3), engine=eng)
    d = bench.make_inputs(np, packed, p5, 1024, seed=8675309 + 5)
    n, m = d["values"].shape
    lbl = np.frombuffer(bytes(bench.LABEL), dtype=np.uint8).copy()
    items = np.zeros(n, dtype=packed._PROVE_ITEM)
    for name in ("values", "blindings", "commitments", "min_values", "min_present", "ext"):
        d[name] = np.ascontiguousarray(d[name])
    items["values"], items["blindings32"], items["commitments32"] = packed._rows(d["values"]), packed._rows(d["blindings"]), packed._rows(d["commitments"])
    items["m"] = m
    items["min_values"], items["min_present"] = packed._rows(d["min_values"]), packed._rows(d["min_present"])
    items["transcript_label"], items["label_len"] = lbl.ctypes.data, len(bench.LABEL)
    items["rng_bytes"], items["rng_len"] = packed._rows(d["ext"]), d["ext"].shape[1]
    plen = 1 + 32 * (3 + 5 + 2 * 8)
    out = np.empty((n, plen), dtype=np.uint8)
    lens = (c_size_t * n)()
    buf = np.empty((n, 203), dtype=np.uint8)
    err = ctypes.create_string_buffer(256)
    ptr = items.ctypes.data_as(POINTER(_lib.ProveItem))

    def call():
        if args.states:
            rc = eng.lib.bpp_prove_batch_mixed_states(eng.ctx, p5.handle, ptr, n, out.ctypes.data, plen, lens, None, buf.ctypes.data, err, 256)
        else:
            rc = eng.lib.bpp_prove_batch_mixed(eng.ctx, p5.handle, ptr, n, out.ctypes.data, plen, lens, None, err, 256)
        assert rc == 0, err.value
    for _ in range(2):
        call()
    lat = []
    for _ in range(args.iters):
        t0 = time.perf_counter()
        call()
        lat.append(time.perf_counter() - t0)
    p5.close()
    eng.close()
    return {"what": "prove", "n": n, "m": m, "states": args.states, "ms_median": round(1e3 * statistics.median(lat), 3), "ms_min": round(1e3 * min(lat), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("verify", "prove"), default="verify")
    ap.add_argument("--states", type=int, default=0)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--wave", type=int, default=-1)
    ap.add_argument("--iters", type=int, default=0, help="timed calls (default: 200 for verify, 8 for prove)")
    args = ap.parse_args()
    args.iters = args.iters or (200 if args.what == "verify" else 8)
    bpp = importlib.import_module("bulletproofs-plus_amd")
    print(json.dumps(verify(args, bpp) if args.what == "verify" else prove(args, bpp)))


if __name__ == "__main__":
    main()
