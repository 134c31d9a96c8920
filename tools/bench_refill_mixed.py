#!/usr/bin/env python3
"""A producer's step of MIXED aggregation factors from device memory: a fresh mixed upload per step against a refill of one resident
batch (bpp_batch_refill_enqueue_mixed, csrc/refill.h).  The sibling of tools/bench_refill.py for the mixed form.

One thread, one context (made on a torch stream), --items slots in the pattern m = 4, 1, 2, 1, 1, 4, 2 at 64 bits, t = 1, promises on
every opening, no nonces; a ring of 4 device input sets of the SAME shape vector (the proved rows rotated inside each class of m), one
of them with one flipped bit in one proof.  Two arms, run alternately in this process after both have been warmed up:

  upload   per step bpp_batch_upload_mixed_device, bpp_verify_enqueue, bpp_batch_destroy -- what a caller of mixed traffic had to
           do every step before the refill existed: the host prelude over proof_lens[] / m[], the allocations, the copy of the row
           table, the read of the result words, the layout planned in the first enqueue
  refill   per step bpp_batch_refill_enqueue_mixed (no proof_lens / m: the batch's own vectors, no count, no mask) and
           bpp_verify_enqueue on one batch

Before anything is timed the refill arm's verdicts are compared with the upload arm's on every input set; a difference ends the run.
Per (arm, repetition) one JSON line: steps/s over a window that ends in a device synchronise, host time of the step's calls (median),
process CPU seconds per step.  The last line is the run's summary; the whole run is APPENDED to --out (profiles/refill_mixed.json: a
list of runs), so that runs of several sizes alternated by tools/gpu_ab.py (--leg cmd) collect in one file:

  tools/gpu_ab.py --leg cmd --cmd "python tools/bench_refill_mixed.py" --reps 3 "--items 1024" "--items 4096"

A record: no ratio is promised and no test asserts a time."""
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

PATTERN = [4, 1, 2, 1, 1, 4, 2]
M_STRIDE, RING = 4, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refill_mixed.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    bpp = importlib.import_module("bulletproofs-plus_amd")
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    _lib = importlib.import_module("bulletproofs-plus_amd._lib")
    n, n_bits, t = args.items, 64, 1
    rows_out = []

    def emit(row):
        rows_out.append(row)
        print(json.dumps(row), flush=True)

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        eng = bpp.Engine(0, stream=stream.cuda_stream)
        params = bpp.RangeParameters.init(n_bits, M_STRIDE, bpp.create_pedersen_gens_with_extension_degree(t), engine=eng)
        ms = np.array([PATTERN[i % 7] for i in range(n)], dtype=np.uint32)
        longest = 1 + 32 * (t + 5 + 2 * ((n_bits * M_STRIDE).bit_length() - 1))
        rows = {"proofs": np.zeros((n, longest), dtype=np.uint8), "commitments": np.zeros((n, M_STRIDE, 32), dtype=np.uint8),
                "min_values": np.zeros((n, M_STRIDE), dtype=np.uint64), "min_present": np.zeros((n, M_STRIDE), dtype=np.uint8)}
        lens = np.zeros(n, dtype=np.uintp)
        rng = np.random.default_rng(20261023)
        classes = {}
        for m in sorted(set(PATTERN)):  # one prove call per class (the array form of the prover takes one m per call)
            idx = np.nonzero(ms == m)[0]
            classes[m] = idx
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
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a.view(np.int64) if a.dtype == np.uint64 else a).copy()).cuda()  # noqa: E731
        ring, bad_slot = [], int(classes[1][min(11, len(classes[1]) - 1)])
        for k in range(RING):  # the same shape vector, other contents: the rows of every class rotated by k places inside the class
            src = np.arange(n)
            for idx in classes.values():
                src[idx] = np.roll(idx, 17 * k)
            pr = rows["proofs"][src].copy()
            if k == 2:
                pr[bad_slot, 1 + 32 * 4 + 5] ^= 2  # one bit of r1 of one m = 1 proof: the final check fails
            ring.append(packed.DeviceMixedInput(dev(pr), lens, ms, dev(rows["commitments"][src]), dev(rows["min_values"][src]),
                                                dev(rows["min_present"][src]), None, bench.LABEL))
        bare = []  # the same arrays without the shape vectors and the transcript fields: what a steady-state refill takes
        for inp in ring:
            st = _lib.MixedBatch.from_buffer_copy(inp.struct)
            st.proof_lens, st.m, st.transcript_state, st.transcript_label, st.label_len = None, None, None, None, 0
            bare.append(st)
        verdicts = [torch.empty((1, 4), dtype=torch.int32, device="cuda") for _ in range(RING)]
        records = [torch.empty((4,), dtype=torch.int32, device="cuda") for _ in range(RING)]
        torch.cuda.synchronize()
        lib, ctx = eng.lib, eng.ctx
        err = ctypes.create_string_buffer(256)
        ticket = ctypes.c_uint64()

        def enqueue(handle, k):
            rc = lib.bpp_verify_enqueue(ctx, handle, None, 0, 0, None, 0, ctypes.c_void_p(verdicts[k].data_ptr()), None, None, ctypes.byref(ticket))
            packed.api._check(rc, ctx)

        def step_upload(k):
            h = ctypes.c_uint64()
            packed.api._check(lib.bpp_batch_upload_mixed_device(ctx, params.handle, ctypes.byref(ring[k].struct), ctypes.byref(h), err, 256), ctx, err)
            enqueue(h, k)
            packed.api._check(lib.bpp_batch_destroy(ctx, h), ctx)

        resident = packed.ResidentBatch.from_mixed(params, ring[0])

        def step_refill(k):
            rc = lib.bpp_batch_refill_enqueue_mixed(ctx, resident.handle, ctypes.byref(bare[k]), None, None, ctypes.c_void_p(records[k].data_ptr()), None)
            packed.api._check(rc, ctx)
            enqueue(resident.handle, k)

        arms = {"upload": step_upload, "refill": step_refill}
        # ---- the refill arm's verdicts against the upload arm's, every input set (this is also the first warm-up)
        seen = {}
        for arm, step in arms.items():
            for k in range(RING):
                step(k)
            torch.cuda.synchronize()
            seen[arm] = [v.cpu().tolist() for v in verdicts]
        if seen["upload"] != seen["refill"] or [v[0][1] for v in seen["upload"]] != [0, 0, 7, 0]:
            raise SystemExit("verdicts differ between the arms, or are not the ones the inputs were made for: %s" % seen)
        if any(r.cpu().tolist() != [0, 0, 0, 1] for r in records):
            raise SystemExit("a refill record is not clean: %s" % [r.cpu().tolist() for r in records])

        def timed(arm, steps):
            step, host = arms[arm], []
            torch.cuda.synchronize()
            c0, t0 = time.process_time(), time.perf_counter()
            for i in range(steps):
                a = time.perf_counter()
                step(i % RING)
                host.append(time.perf_counter() - a)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, statistics.median(host), time.process_time() - c0

        for arm in arms:
            timed(arm, args.warmup)
        r0, e0 = packed.refill_stats(eng), packed.enqueue_stats(eng)
        for rep in range(args.reps):
            for arm in arms:  # alternately
                if arm == "upload":
                    e_before = packed.enqueue_stats(eng)
                wall, host_s, cpu = timed(arm, args.steps)
                if arm == "upload":  # (every fresh batch's first enqueue lays it out and may wait: not the refill arm's)
                    e_after = packed.enqueue_stats(eng)
                    e0 = {k: e0[k] + e_after[k] - e_before[k] for k in e0}
                emit({"arm": arm, "rep": rep, "steps": args.steps, "items_per_step": n, "steps_per_s": round(args.steps / wall, 1),
                      "ms_per_step": round(1e3 * wall / args.steps, 4), "host_ms_per_step_median": round(1e3 * host_s, 4),
                      "cpu_ms_per_step": round(1e3 * cpu / args.steps, 4)})
        r1, e1 = packed.refill_stats(eng), packed.enqueue_stats(eng)
        stats = {"refills": r1["calls"] - r0["calls"], "first_calls": r1["first_calls"] - r0["first_calls"],
                 "refill_host_waits": r1["host_waits"] - r0["host_waits"], "enqueue_host_waits": e1["host_waits"] - e0["host_waits"],
                 "layouts_in_call": e1["layouts_in_call"] - e0["layouts_in_call"]}
        shape = resident.shape()
        resident.close()
        params.close()
        eng.close()
    med = lambda arm, k: statistics.median(r[k] for r in rows_out if r.get("arm") == arm)  # noqa: E731
    run = {"tool": "bench_refill_mixed", "items": n, "n_bits": n_bits, "t": t, "pattern": PATTERN, "ring": RING, "steps": args.steps, "reps": args.reps,
           "m": {str(m): int(len(idx)) for m, idx in classes.items()}, "batch": shape,
           "box": "one %s, HIP %s" % (torch.cuda.get_device_name(0), torch.version.hip), "rows": rows_out, "refill_arm": stats,
           "upload_ms_per_step": med("upload", "ms_per_step"), "refill_ms_per_step": med("refill", "ms_per_step")}
    runs = []
    if os.path.exists(args.out):
        with open(args.out) as f:
            runs = json.load(f)
    runs.append(run)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(runs, f, indent=1)
        f.write("\n")
    print(json.dumps({"tool": "bench_refill_mixed", "items": n, "upload_ms_per_step": run["upload_ms_per_step"],
                      "refill_ms_per_step": run["refill_ms_per_step"], "refill_host_waits": stats["refill_host_waits"],
                      "enqueue_host_waits": stats["enqueue_host_waits"], "layouts_in_call": stats["layouts_in_call"], "box": run["box"]}))


if __name__ == "__main__":
    main()
