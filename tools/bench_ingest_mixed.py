#!/usr/bin/env python3
"""The upload of a batch of MIXED aggregation factors, timed per call WITHOUT the verification:

  items   bpp_batch_upload of the bpp_verify_item array over the rows in page-locked host memory (the host packer of
          csrc/upload_host.h, staging, k_ingest) -- the existing item form, the baseline, not code under test
  device  bpp_batch_upload_mixed_device from the same rows in device memory (csrc/ingest.h: k_ingest_mixed)

on 1024 items -- 512 x m = 1, 256 x m = 2, 256 x m = 4, interleaved -- at 64 bits, t = 1.  The arms alternate in one process as in
tools/bench_ingest.py: both warmed up, then `--reps` rounds of `--inner` calls each (every call followed by bpp_batch_destroy, outside
the timed span).  Per arm: median over rounds of the round's median wall time per call with the lowest and highest round, the
process's CPU time per call and the CPU time of the host worker pool per call.  A record, not a gate: no ratio is asserted anywhere.
Prints one short JSON line; the full record goes to --out (profiles/ingest_mixed.json)."""
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

PATTERN = [1, 2, 1, 4]  # 512 x 1, 256 x 2, 256 x 4 over 1024 items
M_STRIDE = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--items", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_mixed.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    bpp = importlib.import_module("bulletproofs-plus_amd")
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    lib_mod = importlib.import_module("bulletproofs-plus_amd._lib")
    eng = bpp.Engine(0)
    lib = eng.lib
    n_bits, t, n = 64, 1, args.items
    params = bpp.RangeParameters.init(n_bits, M_STRIDE, bpp.create_pedersen_gens_with_extension_degree(t), engine=eng)
    ms = np.array([PATTERN[i % 4] for i in range(n)], dtype=np.uint32)
    longest = 1 + 32 * (t + 5 + 2 * ((n_bits * M_STRIDE).bit_length() - 1))
    rows = {"proofs": np.zeros((n, longest), dtype=np.uint8), "commitments": np.zeros((n, M_STRIDE, 32), dtype=np.uint8),
            "min_values": np.zeros((n, M_STRIDE), dtype=np.uint64), "min_present": np.zeros((n, M_STRIDE), dtype=np.uint8)}
    lens = np.zeros(n, dtype=np.uintp)
    rng = np.random.default_rng(4243)
    for m in sorted(set(PATTERN)):  # one prove call per class (the array form of the prover takes one m per call)
        idx = np.nonzero(ms == m)[0]
        k, rounds = len(idx), (n_bits * m).bit_length() - 1
        values = rng.integers(0, 1 << 63, size=(k, m), dtype=np.uint64)
        one = rng.integers(0, 256, size=(k, m, 32), dtype=np.uint8)
        one[..., 31] &= 0x0f
        one[..., 0] |= 1
        blindings = np.ascontiguousarray(np.repeat(one[:, :, None, :], t, axis=2))
        min_values, min_present = values // np.uint64(3), np.ones((k, m), dtype=np.uint8)
        ext = rng.integers(0, 256, size=(k, 32 * (rounds + 3)), dtype=np.uint8)
        made, proofs = packed.prove(params, values, blindings, None, min_values, min_present, None, bench.LABEL, ext)
        rows["proofs"][idx, :proofs.shape[1]] = proofs
        lens[idx] = proofs.shape[1]
        rows["commitments"][idx, :m] = made
        rows["min_values"][idx, :m] = min_values
        rows["min_present"][idx, :m] = min_present
    pinned = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v).pin_memory() for k, v in rows.items()}
    host = {k: pinned[k].numpy().view(rows[k].dtype) for k in rows}
    addr = lambda a: a.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(a.strides[0])  # noqa: E731
    label = np.frombuffer(bench.LABEL, dtype=np.uint8).copy()
    items = np.zeros(n, dtype=packed._VERIFY_ITEM)
    items["proof"], items["proof_len"], items["commitments32"], items["m"] = addr(host["proofs"]), lens, addr(host["commitments"]), ms
    items["min_values"], items["min_present"] = addr(host["min_values"]), addr(host["min_present"])
    items["transcript_label"], items["label_len"] = label.ctypes.data, len(bench.LABEL)
    dev = packed.DeviceMixedInput(pinned["proofs"].cuda(), lens, ms, pinned["commitments"].cuda(), pinned["min_values"].cuda(),
                                  pinned["min_present"].cuda(), None, bench.LABEL)
    torch.cuda.synchronize()
    err = ctypes.create_string_buffer(256)
    items_p = items.ctypes.data_as(ctypes.POINTER(lib_mod.VerifyItem))

    def one(arm):
        h = ctypes.c_uint64()
        t0 = time.perf_counter()
        if arm == "items":
            rc = lib.bpp_batch_upload(eng.ctx, params.handle, items_p, n, ctypes.byref(h), err, 256)
        else:
            rc = lib.bpp_batch_upload_mixed_device(eng.ctx, params.handle, ctypes.byref(dev.struct), ctypes.byref(h), err, 256)
        dt = time.perf_counter() - t0
        assert rc == 0, (arm, rc, err.value)
        assert lib.bpp_batch_destroy(eng.ctx, h) == 0
        return dt

    arms = ("items", "device")
    # the batch the device form makes verifies: checked once, outside the timed part
    rb = packed.ResidentBatch.from_mixed(params, dev)
    rb.verify_only(0)
    shapes = [rb.shape()]
    rb.close()
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
    record = {"shape": {"n_bits": n_bits, "t": t, "items": n, "m": {str(m): int((ms == m).sum()) for m in sorted(set(PATTERN))}, "batch": shapes[0]},
              "reps": args.reps, "inner": args.inner, "host_threads": bpp.host_threads()}
    for arm, v in per.items():
        record[arm] = {"ms": statistics.median(v["rounds_ms"]), "lo": min(v["rounds_ms"]), "hi": max(v["rounds_ms"]),
                       "cpu_ms_per_call": statistics.median(v["cpu_ms"]), "pool_cpu_ms_per_call": statistics.median(v["pool_cpu_ms"])}
    record["ingest_stats"] = dict(zip(("device_calls", "host_fallback_calls", "fallback_bytes"), packed.ingest_stats(eng)))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(record) + "\n")
    print(json.dumps({"tool": "bench_ingest_mixed", "items": n, "items_ms": round(record["items"]["ms"], 3),
                      "device_ms": round(record["device"]["ms"], 3)}))
    params.close()
    eng.close()


if __name__ == "__main__":
    main()
