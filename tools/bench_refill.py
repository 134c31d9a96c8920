#!/usr/bin/env python3
"""A producer's step from device memory: a fresh upload per step against a refill of one resident batch (bpp_batch_refill_enqueue).

One thread, one context (made on a torch stream, so that torch events can bracket the engine's work), a ring of 4 device input sets
of 1024 proofs (m = 1, 64 bits, no nonces), one of them tampered.  Two arms, run alternately in ONE process after both have been
warmed up, as tools/gpu_ab.py alternates its arms:

  upload   per step bpp_batch_upload_packed_device, bpp_verify_enqueue, bpp_batch_destroy
  refill   per step bpp_batch_refill_enqueue and bpp_verify_enqueue on one batch
  refill_count_K   (one per --count K, any number of them) per step bpp_batch_refill_enqueue_count with the live count K in a device
           word and bpp_verify_enqueue on a batch of its own: what a step costs when N - K of its slots are dead.  A dead slot passes
           through the per-proof kernels with weight zero, so these arms state a cost; they are not there to meet a bar.
  refill_live_D    (one per --live D, a density in [0, 1]) per step bpp_batch_refill_enqueue_live under a random mask with exactly
           L = round(D * 1024) live slots, a different mask for every input set of the ring, on a batch of its own; every --live D also
           adds the arm refill_count_L, the count form at the same number of live items, so that the two alternate in this process.
           Neither skips dead slots; the mask form's extra work is a byte per slot in four kernels and a ballot per 64 slots in the
           weight chain.  The last line states, per density, both arms' time per step over the repetitions and whether the mask arm's
           median lies inside the count arm's own spread (its lowest to its highest repetition).  Without --out the rows go to
           profiles/refill_live.json.

Per (arm, repetition) one JSON line: steps/s over a window that ends in a device synchronise, process CPU seconds per step, host time
of the step's calls (median).  In a pass of its own (not inside the timed window) every step's ingest part is bracketed by events on
the stream: for the upload arm the span of the whole blocking upload call as the device sees it (k_ingest_packed, the copy of its
result words, the host's plan in between, the packing kernels, the commitments' decompression); for the refill arm k_refill_packed,
k_refill_finish and the same decompression.  The kernels alone come from a kernel trace of this program (rocprofv3 --kernel-trace
--stats -- python tools/bench_refill.py ...): --kernel-stats CSV adds the rows of k_ingest_packed, k_refill_packed and k_refill_finish.
Before anything is timed the refill arm's verdicts are compared with the upload arm's on every input set; a difference ends the run.
The refill arm's host_waits (bpp_refill_stats, bpp_enqueue_stats) are reported: the feature's claim is that they stay 0.
--out FILE collects the lines (profiles/refill.json)."""
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
    ap.add_argument("--event-steps", type=int, default=40)
    ap.add_argument("--kernel-stats", default="", help="a rocprofv3 kernel_stats.csv of a run of this program")
    ap.add_argument("--count", type=int, action="append", default=[], help="add an arm that refills with this live count (repeatable)")
    ap.add_argument("--live", type=float, action="append", default=[], help="add an arm that refills under a random mask of this density, and the count arm of as many live items (repeatable)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.live and not args.out:
        args.out = os.path.join(ROOT, "profiles", "refill_live.json")
    live_counts = {D: int(round(D * N)) for D in args.live}
    for D, L in live_counts.items():
        if not 0 <= L <= N:
            raise SystemExit("--live %s: a density in [0, 1] expected" % D)
        if L not in args.count:
            args.count.append(L)
    import numpy as np
    import torch
    import bench
    from tests.helpers import LABEL
    bpp = importlib.import_module("bulletproofs-plus_amd")
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    _lib = importlib.import_module("bulletproofs-plus_amd._lib")
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
        ring = [packed.DevicePackedInput(dev(proofs[k * N:(k + 1) * N]), dev(d["commitments"][k * N:(k + 1) * N]),
                                         dev(d["min_values"][k * N:(k + 1) * N]), dev(d["min_present"][k * N:(k + 1) * N]), None, LABEL)
                for k in range(RING)]
        bare = []  # the same arrays without the transcript fields: what a refill takes
        for inp in ring:
            st = _lib.PackedBatch.from_buffer_copy(inp.struct)
            st.transcript_state, st.transcript_label, st.label_len = None, None, 0
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

        def step_upload(k, mark=None):
            h = ctypes.c_uint64()
            if mark:
                mark[0].record(stream)
            packed.api._check(lib.bpp_batch_upload_packed_device(ctx, params.handle, ctypes.byref(ring[k].struct), ctypes.byref(h), err, 256), ctx, err)
            if mark:
                mark[1].record(stream)
            enqueue(h, k)
            packed.api._check(lib.bpp_batch_destroy(ctx, h), ctx)

        resident = packed.ResidentBatch(params, ring[0], None, None, None, None, LABEL, form="device")

        def step_refill(k, mark=None):
            if mark:
                mark[0].record(stream)
            rc = lib.bpp_batch_refill_enqueue(ctx, resident.handle, ctypes.byref(bare[k]), ctypes.c_void_p(records[k].data_ptr()), None)
            packed.api._check(rc, ctx)
            if mark:
                mark[1].record(stream)
            enqueue(resident.handle, k)

        arms = {"upload": step_upload, "refill": step_refill}
        counted = {}
        for K in args.count:  # one batch and one count word per arm
            rb = packed.ResidentBatch(params, ring[0], None, None, None, None, LABEL, form="device")
            word = torch.tensor([K], dtype=torch.int32, device="cuda")

            def step_count(k, mark=None, rb=rb, word=word):
                if mark:
                    mark[0].record(stream)
                rc = lib.bpp_batch_refill_enqueue_count(ctx, rb.handle, ctypes.byref(bare[k]), ctypes.c_void_p(word.data_ptr()),
                                                        ctypes.c_void_p(records[k].data_ptr()), None)
                packed.api._check(rc, ctx)
                if mark:
                    mark[1].record(stream)
                enqueue(rb.handle, k)

            counted["refill_count_%d" % K] = (K, rb, word, step_count)
        masked = {}
        for D, L in live_counts.items():  # one batch per arm and one mask per input set, each with exactly L live slots
            rb = packed.ResidentBatch(params, ring[0], None, None, None, None, LABEL, form="device")
            gen = np.random.default_rng(int(D * 1e6) + 17)
            host_masks = []
            for _k in range(RING):
                mk = np.zeros(N, dtype=np.uint8)
                mk[gen.permutation(N)[:L]] = 1
                host_masks.append(mk)
            dev_masks = [torch.from_numpy(mk).cuda() for mk in host_masks]

            def step_live(k, mark=None, rb=rb, dev_masks=dev_masks):
                if mark:
                    mark[0].record(stream)
                rc = lib.bpp_batch_refill_enqueue_live(ctx, rb.handle, ctypes.byref(bare[k]), ctypes.c_void_p(dev_masks[k].data_ptr()),
                                                       ctypes.c_void_p(records[k].data_ptr()), None)
                packed.api._check(rc, ctx)
                if mark:
                    mark[1].record(stream)
                enqueue(rb.handle, k)

            masked["refill_live_%g" % D] = (L, rb, host_masks, dev_masks, step_live)
        torch.cuda.synchronize()
        # ---- the refill arm's verdicts against the upload arm's, every input set (this is also the first warm-up)
        seen = {}
        for arm, step in arms.items():
            for k in range(RING):
                step(k)
            torch.cuda.synchronize()
            seen[arm] = [v.cpu().tolist() for v in verdicts]
        if seen["upload"] != seen["refill"] or [v[0][1] for v in seen["upload"]] != [0, 0, 7, 0]:
            raise SystemExit("verdicts differ between the arms, or are not the ones the inputs were made for: %s" % seen)
        for arm, (K, rb, word, step) in counted.items():  # the tampered proof is item 77 of set 2: live or not
            for k in range(RING):
                step(k)
            torch.cuda.synchronize()
            got = [v.cpu().tolist()[0] for v in verdicts]
            want = [[0, 0, 0, 1 if 0 < K <= N else (9 if K == 0 else 5)] for _ in range(RING)]
            if 77 < K <= N:
                want[2] = [1, 7, 0, 1]
            if got != want:
                raise SystemExit("%s: verdicts %s, expected %s" % (arm, got, want))
            arms[arm] = step
        for arm, (L, rb, host_masks, _dev_masks, step) in masked.items():  # the tampered proof is item 77 of set 2: live or not
            for k in range(RING):
                step(k)
            torch.cuda.synchronize()
            got = [v.cpu().tolist()[0] for v in verdicts]
            want = [[0, 0, 0, 1 if L else 9] for _ in range(RING)]
            if host_masks[2][77]:
                want[2] = [1, 7, 0, 1]
            if got != want:
                raise SystemExit("%s: verdicts %s, expected %s" % (arm, got, want))
            arms[arm] = step

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
                emit({"arm": arm, "rep": rep, "steps": args.steps, "proofs_per_step": N, "steps_per_s": round(args.steps / wall, 1),
                      "ms_per_step": round(1e3 * wall / args.steps, 4), "host_ms_per_step_median": round(1e3 * host_s, 4),
                      "cpu_ms_per_step": round(1e3 * cpu / args.steps, 4)})
        r1, e1 = packed.refill_stats(eng), packed.enqueue_stats(eng)
        emit({"refill_arm": {"refills": r1["calls"] - r0["calls"], "first_calls": r1["first_calls"] - r0["first_calls"],
                             "refill_host_waits": r1["host_waits"] - r0["host_waits"], "enqueue_host_waits": e1["host_waits"] - e0["host_waits"],
                             "layouts_in_call": e1["layouts_in_call"] - e0["layouts_in_call"]}})
        # ---- the ingest part of a step as the device sees it, from events, one step at a time
        for arm, step in arms.items():
            spans = []
            for i in range(args.event_steps):
                mark = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                step(i % RING, mark)
                torch.cuda.synchronize()
                spans.append(mark[0].elapsed_time(mark[1]))
            emit({"arm": arm, "ingest_span_ms_median": round(statistics.median(spans), 4), "ingest_span_ms_min": round(min(spans), 4),
                  "what": "events around bpp_batch_upload_packed_device" if arm == "upload" else "events around bpp_batch_refill_enqueue"})
        # ---- the mask form against the count form at the same number of live items: is it inside the count arm's own spread
        for arm, (L, _rb, _hm, _dm, _step) in masked.items():
            mine = [r["ms_per_step"] for r in rows if r.get("arm") == arm and "ms_per_step" in r]
            theirs = [r["ms_per_step"] for r in rows if r.get("arm") == "refill_count_%d" % L and "ms_per_step" in r]
            if mine and theirs:
                emit({"live_against_count": arm, "live_items": L, "count_arm": "refill_count_%d" % L,
                      "live_ms_per_step": mine, "count_ms_per_step": theirs, "live_ms_per_step_median": round(statistics.median(mine), 4),
                      "count_ms_per_step_median": round(statistics.median(theirs), 4), "count_ms_per_step_spread": [min(theirs), max(theirs)],
                      "live_median_inside_count_spread": bool(statistics.median(mine) <= max(theirs))})
        resident.close()
        for _K, rb, _word, _step in counted.values():
            rb.close()
        for _L, rb, _hm, _dm, _step in masked.values():
            rb.close()
        params.close()
        eng.close()
    if args.kernel_stats:
        with open(args.kernel_stats) as f:
            for r in csv.DictReader(f):
                name = r.get("Name") or r.get("KernelName") or ""
                if any(k in name for k in ("k_ingest_packed", "k_refill_packed", "k_refill_finish")):
                    emit({"kernel": name.split("(")[0], "calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 3),
                          "min_us": round(float(r["MinNs"]) / 1e3, 3), "max_us": round(float(r["MaxNs"]) / 1e3, 3)})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
