#!/usr/bin/env python3
"""The upload of a packed batch, host form against device form, timed per call WITHOUT the verification:

  host    bpp_batch_upload_packed from page-locked host arrays (the host packer of csrc/upload_host.h, staging, k_ingest)
  device  bpp_batch_upload_packed_device from arrays that already lie in device memory (csrc/ingest.h: k_ingest_packed)

on the BASELINE shape (m = 1, t = 1, 64 bits) at 64 x 1024 proofs and at one 1024-proof call.  Both arms are warmed up, then timed
in turn, `--reps` rounds of `--inner` calls each (every call followed by bpp_batch_destroy, outside the timed span: the next upload
adopts the buffers, as in a service that verifies call after call).  Per arm: median over rounds of the round's median wall time per
call with the lowest and highest round, the process's CPU time per call and the CPU time of the host worker pool per call
(bpp_host_pool_cpu_ns).  A record, not a gate: no ratio is asserted anywhere.  Prints one short JSON line; the full record goes to
--out (profiles/ingest.json)."""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [64 * 1024, 1024]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--made", type=int, default=4096, help="distinct proofs made by the prover; larger batches repeat them")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    bpp = importlib.import_module("bulletproofs-plus_amd")
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    eng = bpp.Engine(0)
    lib = eng.lib
    params = bpp.RangeParameters.init(64, 1, bpp.create_pedersen_gens_with_extension_degree(1), engine=eng)
    made = bench.make_inputs(np, packed, params, args.made, seed=4242)
    record = {"shape": {"n_bits": 64, "m": 1, "t": 1}, "reps": args.reps, "inner": args.inner, "host_threads": bpp.host_threads(), "sizes": []}
    for n in SIZES:
        idx = np.arange(n) % args.made
        arrays = {k: np.ascontiguousarray(made[k][idx]) for k in ("proofs", "commitments", "min_values", "min_present", "seeds")}
        pinned = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v).pin_memory() for k, v in arrays.items()}
        host = packed.PackedInput(*[pinned[k].numpy().view(arrays[k].dtype) for k in ("proofs", "commitments", "min_values", "min_present", "seeds")],
                                  bench.LABEL)
        dev = packed.DevicePackedInput(*[pinned[k].cuda() for k in ("proofs", "commitments", "min_values", "min_present", "seeds")],
                                       bench.LABEL)
        torch.cuda.synchronize()
        err = ctypes.create_string_buffer(256)
        arms = {"host": (lib.bpp_batch_upload_packed, host), "device": (lib.bpp_batch_upload_packed_device, dev)}

        def one(arm):
            fn, inp = arms[arm]
            h = ctypes.c_uint64()
            t0 = time.perf_counter()
            rc = fn(eng.ctx, params.handle, ctypes.byref(inp.struct), ctypes.byref(h), err, 256)
            dt = time.perf_counter() - t0
            assert rc == 0, (arm, rc, err.value)
            assert lib.bpp_batch_destroy(eng.ctx, h) == 0
            return dt

        for arm in arms:
            for _ in range(3):
                one(arm)
        per = {arm: {"rounds_ms": [], "cpu_ms": [], "pool_cpu_ms": []} for arm in arms}
        for _ in range(args.reps):
            for arm in arms:
                c0, p0 = time.process_time(), lib.bpp_host_pool_cpu_ns()
                ts = [one(arm) for _ in range(args.inner)]
                c1, p1 = time.process_time(), lib.bpp_host_pool_cpu_ns()
                per[arm]["rounds_ms"].append(statistics.median(ts) * 1e3)
                per[arm]["cpu_ms"].append((c1 - c0) * 1e3 / args.inner)  # (the destroy between the calls included)
                per[arm]["pool_cpu_ms"].append((p1 - p0) * 1e-6 / args.inner)
        row = {"proofs": n}
        for arm, v in per.items():
            row[arm] = {"ms": statistics.median(v["rounds_ms"]), "lo": min(v["rounds_ms"]), "hi": max(v["rounds_ms"]),
                        "cpu_ms_per_call": statistics.median(v["cpu_ms"]), "pool_cpu_ms_per_call": statistics.median(v["pool_cpu_ms"])}
        record["sizes"].append(row)
    record["ingest_stats"] = dict(zip(("device_calls", "host_fallback_calls", "fallback_bytes"), packed.ingest_stats(eng)))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(record) + "\n")
    print(json.dumps({"tool": "bench_ingest", "sizes": [{"proofs": r["proofs"], "host_ms": round(r["host"]["ms"], 3),
                                                         "device_ms": round(r["device"]["ms"], 3)} for r in record["sizes"]]}))
    params.close()
    eng.close()


if __name__ == "__main__":
    main()
