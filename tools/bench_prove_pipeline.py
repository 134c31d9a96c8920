#!/usr/bin/env python3
"""Prove calls in flight from ONE thread (bpp_prove_submit / bpp_prove_collect) against one blocking call at a time and against a
context and a thread per call in flight: BASELINE configs[4]'s shape (1024 x aggregation-4, extension degree 3, 64-bit) per call,
32 calls after 4 warm-up calls.  One JSON line: proofs/s, median and p99 ms per call, the hardware queues the runtime has.

  --arm blocking                     one bpp_prove_batch_mixed at a time
  --arm pipeline --depth {1,2,3,4}   one thread, as many tickets outstanding as lanes
  --arm threads --threads 4          a context and a thread per call in flight (what tools/bench_prove_concurrent.py does)
  --nonces                           1024 x m = 1 with seed nonces instead, at extension degree --t (default 3, as
                                     tools/bench_prover_leg.py --nonces)
  --check                            "prove_check" = 1, set before the lanes exist

Every proof of the first call of the arm is compared byte for byte with the blocking call's.  GPU_MAX_HW_QUEUES is taken as found.
A/B: tools/gpu_ab.py --leg cmd --cmd "python3 tools/bench_prove_pipeline.py" "--arm blocking" "--arm pipeline --depth 2" ..."""
import argparse
import ctypes
import importlib
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_PROOFS = 1024


def item_array(np, packed, _lib, d, m, label):
    """the bpp_prove_item array over the arrays of bench.make_inputs (the caller keeps `d` and the returned objects alive)"""
    n = d["values"].shape[0]
    lbl = np.frombuffer(bytes(label), dtype=np.uint8).copy()
    items = np.zeros(n, dtype=packed._PROVE_ITEM)
    items["values"] = packed._rows(d["values"])
    items["blindings32"] = packed._rows(d["blindings"])
    items["commitments32"] = packed._rows(d["commitments"])
    items["m"] = m
    items["min_values"] = packed._rows(d["min_values"])
    items["min_present"] = packed._rows(d["min_present"])
    if d["seeds"] is not None:
        items["seed_nonce32"] = packed._rows(d["seeds"])
    items["transcript_label"] = lbl.ctypes.data
    items["label_len"] = len(label)
    items["rng_bytes"] = packed._rows(d["ext"])
    items["rng_len"] = d["ext"].shape[1]
    return items, lbl, items.ctypes.data_as(ctypes.POINTER(_lib.ProveItem))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--arm", choices=("blocking", "pipeline", "threads"), default="blocking")
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--threads", type=int, default=4)
    ap.add_argument("--calls", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--nonces", action="store_true")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--t", type=int, default=3, help="extension degree of the --nonces proofs")
    a = ap.parse_args()
    import numpy as np
    bpp = importlib.import_module("bulletproofs-plus_amd")
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    _lib = bpp._lib
    import bench
    m, t = (1, a.t) if a.nonces else (4, 3)
    eng = bpp.Engine(0)
    lib = eng.lib
    if a.check:
        eng.set_option("prove_check", 1)
        if a.nonces:
            eng.set_option("prove_check_recovery", 1)
    params = bpp.RangeParameters.init(64, m, bpp.create_pedersen_gens_with_extension_degree(t), engine=eng)
    d = bench.make_inputs(np, packed, params, N_PROOFS, seed=99)  # also builds the fixed-base table
    items, _lbl, arr = item_array(np, packed, _lib, d, m, bench.LABEL)
    rounds = (64 * m).bit_length() - 1
    plen = 1 + 32 * (t + 5 + 2 * rounds)

    def outputs():
        return np.empty((N_PROOFS, plen), dtype=np.uint8), (ctypes.c_size_t * N_PROOFS)(), ctypes.create_string_buffer(256)

    def blocking(e):
        out, lens, err = outputs()
        rc = lib.bpp_prove_batch_mixed(e.ctx, params.handle, arr, N_PROOFS, out.ctypes.data, plen, lens, None, err, 256)
        if rc != 0:
            raise SystemExit("bpp_prove_batch_mixed: %d %s" % (rc, err.value))
        return out

    def submit():
        ticket = ctypes.c_uint64()
        err = ctypes.create_string_buffer(256)
        rc = lib.bpp_prove_submit(eng.ctx, params.handle, arr, N_PROOFS, plen, 0, 0, ctypes.byref(ticket), err, 256)
        if rc != 0:
            raise SystemExit("bpp_prove_submit: %d %s" % (rc, err.value))
        return ticket.value

    def collect(ticket):
        out, lens, err = outputs()
        rc = lib.bpp_prove_collect(eng.ctx, ticket, None, out.ctypes.data, lens, None, err, 256)
        if rc != 0:
            raise SystemExit("bpp_prove_collect: %d %s" % (rc, err.value))
        return out

    def same_as_blocking(got):
        if not np.array_equal(got, reference):
            raise SystemExit("the first call's proofs differ from the blocking call's")
        return True

    reference = blocking(eng)  # (the blocking call's bytes; also warms the context)
    first_equal = same_as_blocking(d["proofs"])  # (bpp_prove_batch's, which made the inputs)
    per_call = []  # ms from a call's submission to its result
    if a.arm == "blocking":
        for _ in range(a.warmup):
            blocking(eng)
        t0 = time.perf_counter()
        for _ in range(a.calls):
            s = time.perf_counter()
            blocking(eng)
            per_call.append(1e3 * (time.perf_counter() - s))
        elapsed = time.perf_counter() - t0
        in_flight = 1
    elif a.arm == "pipeline":
        api_rc = lib.bpp_prove_pipeline_depth(eng.ctx, a.depth)
        if api_rc != 0:
            raise SystemExit("bpp_prove_pipeline_depth: %d" % api_rc)
        first_equal = same_as_blocking(collect(submit()))
        for _ in range(a.warmup):  # every lane's arena and streams
            for tk in [submit() for _ in range(a.depth)]:
                collect(tk)
        queue = []
        t0 = time.perf_counter()
        for _ in range(a.calls):
            if len(queue) == a.depth:  # as many tickets outstanding as lanes: take the oldest, hand in the next
                tk, s = queue.pop(0)
                collect(tk)
                per_call.append(1e3 * (time.perf_counter() - s))
            s = time.perf_counter()
            queue.append((submit(), s))
        for tk, s in queue:
            collect(tk)
            per_call.append(1e3 * (time.perf_counter() - s))
        elapsed = time.perf_counter() - t0
        in_flight = a.depth
    else:
        engs = [bpp.Engine(0) for _ in range(a.threads)]
        for e in engs:
            if a.check:
                e.set_option("prove_check", 1)
                if a.nonces:
                    e.set_option("prove_check_recovery", 1)
            params.share(e)
        first_equal = same_as_blocking(blocking(engs[0]))
        for e in engs:
            for _ in range(a.warmup):
                blocking(e)
        share = [a.calls // a.threads + (1 if k < a.calls % a.threads else 0) for k in range(a.threads)]
        times = [[] for _ in engs]

        def worker(k):
            for _ in range(share[k]):
                s = time.perf_counter()
                blocking(engs[k])
                times[k].append(1e3 * (time.perf_counter() - s))
        th = [threading.Thread(target=worker, args=(k,)) for k in range(a.threads)]
        t0 = time.perf_counter()
        for x in th:
            x.start()
        for x in th:
            x.join()
        elapsed = time.perf_counter() - t0
        per_call = [x for row in times for x in row]
        in_flight = a.threads
    info = packed.runtime_info(eng)
    stats = eng.prove_check_stats() if a.check else None
    if a.arm == "threads" and a.check:
        for e in engs:
            s = e.prove_check_stats()
            stats = {k: stats[k] + s[k] for k in stats}
    per_call.sort()
    print(json.dumps({"metric": "range proofs created/sec (batch), prove calls in flight", "arm": a.arm, "in_flight": in_flight,
                      "aggregation": m, "extension_degree": t, "seed_nonces": bool(a.nonces), "proofs_per_call": N_PROOFS,
                      "calls": a.calls, "proofs_per_s": N_PROOFS * a.calls / elapsed, "ms_per_call_median": per_call[len(per_call) // 2],
                      "ms_per_call_p99": per_call[min(len(per_call) - 1, int(0.99 * len(per_call)))],
                      "ms_per_call_throughput": 1e3 * elapsed / a.calls, "prove_check": 1 if a.check else 0,
                      "check_stats": stats, "hw_queues": info["hw_queues"], "contexts": info["contexts"],
                      "first_call_equals_blocking": first_equal}))
    if a.arm == "threads":
        for e in engs:
            e.close()
    eng.close()


if __name__ == "__main__":
    main()
