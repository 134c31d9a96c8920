#!/usr/bin/env python3
"""What per-item transcripts cost in a producer's step: refill with transcripts + bpp_verify_enqueue_states against the existing
refill + bpp_verify_enqueue, at the shape of tools/bench_refill.py (1024 items, 64 bits, m = 1, t = 1, a ring of 4 device input sets,
one of them with one flipped bit in one proof), on the same tree, one thread, one context made on a torch stream.

Two resident batches of the same arrays, two arms, run alternately in this process after both have been warmed up:

  plain        per step bpp_batch_refill_enqueue and bpp_verify_enqueue on a batch of bpp_batch_upload_packed_device
  transcripts  per step bpp_batch_refill_enqueue_transcripts (no count, no mask) and bpp_verify_enqueue_states on a batch of
               bpp_batch_upload_packed_device_transcripts: 203 more bytes per proof in (k_item_states), PASS 1 in its STATES form,
               203 bytes per proof out (k_states_out)

The proofs are bench.py's, proved under the one label; every row of the state array is that label's fresh transcript, so both arms
verify the same proofs to the same verdicts (held to each other before anything is timed; the state rows of the valid sets must be
non-zero and those of the set with the invalid proof zero).  What is measured is the extra bytes and kernels, which do not depend on
what the rows hold.

Per (arm, repetition) one JSON line: steps/s over a window that ends in a device synchronise, host time of the step's calls (median),
process CPU seconds per step.  --kernel-stats FILE adds the rows of k_item_states and k_states_out (and of the two PASS-1 forms) from
a rocprofv3 kernel_stats.csv of a run of this program (kernel tracing alone: `rocprofv3 --kernel-trace --stats -- python
tools/bench_item_transcripts.py --steps 40 --reps 1`).  The last line is the summary: the medians and their difference.  The rows go
under "step" of --out (profiles/item_transcripts.json), beside the A/B runs of tools/bench_refill.py and bench.py against the parent
commit's library that tools/gpu_ab.py made.  A record: no figure is promised and no test asserts a time."""
import argparse
import csv
import ctypes
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, RING = 1024, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-stats", default="", help="a rocprofv3 kernel_stats.csv of a run of this program")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "item_transcripts.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from tests.helpers import LABEL
    bpp = importlib.import_module("bulletproofs-plus_amd")
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        eng = bpp.Engine(0, stream=stream.cuda_stream)
        params = bpp.RangeParameters.init(64, 1, bpp.create_pedersen_gens_with_extension_degree(1), engine=eng)
        d = bench.make_inputs(np, packed, params, N * RING, seed=20261020)
        proofs = d["proofs"].copy()
        proofs[2 * N + 77, 1 + 32 + 96 + 5] ^= 2  # set 2: one bit of r1 of one proof, the final check fails
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a.view(np.int64) if a.dtype == np.uint64 else a).copy()).cuda()  # noqa: E731
        fresh = np.frombuffer(bpp.Transcript.new(LABEL).strobe_state(), dtype=np.uint8)
        state_rows = dev(np.repeat(fresh[None, :], N, axis=0))

        def ring_of(**kw):
            return [packed.DevicePackedInput(dev(proofs[k * N:(k + 1) * N]), dev(d["commitments"][k * N:(k + 1) * N]),
                                             dev(d["min_values"][k * N:(k + 1) * N]), dev(d["min_present"][k * N:(k + 1) * N]), None, LABEL, **kw)
                    for k in range(RING)]

        rings = {"plain": ring_of(), "transcripts": ring_of(item_states=state_rows)}
        bare = {arm: [inp.struct_without_transcript() for inp in ring] for arm, ring in rings.items()}
        verdicts = {arm: [torch.empty((1, 4), dtype=torch.int32, device="cuda") for _ in range(RING)] for arm in rings}
        records = {arm: [torch.empty((4,), dtype=torch.int32, device="cuda") for _ in range(RING)] for arm in rings}
        states_out = [torch.empty((N, 203), dtype=torch.uint8, device="cuda") for _ in range(RING)]
        torch.cuda.synchronize()
        lib, ctx = eng.lib, eng.ctx
        ticket = ctypes.c_uint64()
        resident = {arm: packed.ResidentBatch(params, ring[0], None, None, None, None, LABEL, form="device") for arm, ring in rings.items()}

        def step_plain(k):
            h = resident["plain"].handle
            packed.api._check(lib.bpp_batch_refill_enqueue(ctx, h, ctypes.byref(bare["plain"][k]), ctypes.c_void_p(records["plain"][k].data_ptr()), None), ctx)
            rc = lib.bpp_verify_enqueue(ctx, h, None, 0, 0, None, 0, ctypes.c_void_p(verdicts["plain"][k].data_ptr()), None, None, ctypes.byref(ticket))
            packed.api._check(rc, ctx)

        def step_transcripts(k):
            h = resident["transcripts"].handle
            rc = lib.bpp_batch_refill_enqueue_transcripts(ctx, h, ctypes.byref(bare["transcripts"][k]), rings["transcripts"][k].item_states, None, None,
                                                          ctypes.c_void_p(records["transcripts"][k].data_ptr()), None)
            packed.api._check(rc, ctx)
            rc = lib.bpp_verify_enqueue_states(ctx, h, None, 0, 0, None, 0, ctypes.c_void_p(verdicts["transcripts"][k].data_ptr()), None, None,
                                               ctypes.c_void_p(states_out[k].data_ptr()), ctypes.byref(ticket))
            packed.api._check(rc, ctx)

        arms = {"plain": step_plain, "transcripts": step_transcripts}
        # ---- the arms' verdicts against each other, every input set (this is also the first warm-up)
        seen = {}
        for arm, step in arms.items():
            for k in range(RING):
                step(k)
            torch.cuda.synchronize()
            seen[arm] = [v.cpu().tolist() for v in verdicts[arm]]
            if any(r.cpu().tolist() != [0, 0, 0, 1] for r in records[arm]):
                raise SystemExit("a refill record is not clean: %s" % [r.cpu().tolist() for r in records[arm]])
        if seen["plain"] != seen["transcripts"] or [v[0][1] for v in seen["plain"]] != [0, 0, 7, 0]:
            raise SystemExit("verdicts differ between the arms, or are not the ones the inputs were made for: %s" % seen)
        given = [bool(s.any(dim=1).all().item()) for s in states_out]
        if given != [True, True, False, True] or states_out[2].any().item():
            raise SystemExit("state rows: non-zero rows expected for the valid sets and zero rows for the rejected one, got %s" % given)

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
                wall, host_s, cpu = timed(arm, args.steps)
                emit({"arm": arm, "rep": rep, "steps": args.steps, "items_per_step": N, "steps_per_s": round(args.steps / wall, 1),
                      "ms_per_step": round(1e3 * wall / args.steps, 4), "host_ms_per_step_median": round(1e3 * host_s, 4),
                      "cpu_ms_per_step": round(1e3 * cpu / args.steps, 4)})
        r1, e1 = packed.refill_stats(eng), packed.enqueue_stats(eng)
        stats = {"refills": r1["calls"] - r0["calls"], "first_calls": r1["first_calls"] - r0["first_calls"],
                 "refill_host_waits": r1["host_waits"] - r0["host_waits"], "enqueue_host_waits": e1["host_waits"] - e0["host_waits"],
                 "layouts_in_call": e1["layouts_in_call"] - e0["layouts_in_call"]}
        for rb in resident.values():
            rb.close()
        params.close()
        eng.close()
    if args.kernel_stats:
        with open(args.kernel_stats) as f:
            for r in csv.DictReader(f):
                name = r.get("Name") or r.get("KernelName") or ""
                if any(k in name for k in ("k_item_states", "k_states_out", "k_transcripts", "k_refill_packed")):
                    emit({"kernel": name.split("(")[0], "calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 3),
                          "min_us": round(float(r["MinNs"]) / 1e3, 3), "max_us": round(float(r["MaxNs"]) / 1e3, 3)})
    med = lambda arm: statistics.median(r["ms_per_step"] for r in rows if r.get("arm") == arm)  # noqa: E731
    span = lambda arm: [min(r["ms_per_step"] for r in rows if r.get("arm") == arm), max(r["ms_per_step"] for r in rows if r.get("arm") == arm)]  # noqa: E731
    summary = {"tool": "bench_item_transcripts", "items": N, "steps": args.steps, "reps": args.reps, "plain_ms_per_step": med("plain"),
               "transcripts_ms_per_step": med("transcripts"), "difference_ms_per_step": round(med("transcripts") - med("plain"), 4),
               "plain_range_ms": span("plain"), "transcripts_range_ms": span("transcripts"), "steady_state": stats,
               "box": "one %s, HIP %s" % (torch.cuda.get_device_name(0), torch.version.hip)}
    emit(summary)
    if args.out:  # the file's "step" rows are this run's; what else it holds (the A/B runs against the parent commit) stays
        doc = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                doc = json.load(f)
        doc["step"] = rows
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
