#!/usr/bin/env python3
"""Proving on the stream from a resident plan (bpp_prove_enqueue) against the blocking bpp_prove_openings_device, timed per step in
one process, the arms alternating:

  blocking          bpp_prove_openings_device on arrays in device memory: plans, stages, launches, waits (the existing form)
  enqueue           plan.enqueue -> ticket wait on the same arrays (the plan made once, outside the timed span)
  blocking+verify   blocking prove -> bpp_batch_upload_mixed_device -> bpp_verify_resident -> bpp_batch_destroy
  enqueue+verify    plan.enqueue -> bpp_batch_refill_enqueue_mixed(live = the prover's ok mask) -> bpp_verify_enqueue -> ONE wait,
                    from one thread on one resident batch

Two shapes: configs[4] (1024 x m = 4, t = 3, 64 bits) and 1024 x m = 1, t = 3, a seed nonce on each item.  Per arm: the median over
`--reps` rounds of the round's median wall time per step (lowest and highest round), proofs/s, the wall time until the step's calls
had returned (`host_ms_in_calls`: what a service's thread is not free for -- the whole step in a blocking arm, the enqueues alone
in the others) and the calling thread's CPU time over the whole step, its wait included (bpp_enqueue_wait is the runtime's
spinning event wait; the blocking call naps through most of its own).  The counters of
bpp_prove_enqueue_stats, bpp_refill_stats and bpp_enqueue_stats go into the record: the steady state allocates nothing and waits for
nothing inside the calls.  A record, not a gate: no figure is asserted anywhere.  The expectation is equal GPU time and lower host
time for the enqueue arms, not a speed-up: the kernels are the same.

--arms blocking: the blocking arm alone (runs on an older build of the library named by BPP_LIB_PATH as well: the parent-commit arm
of tools/gpu_ab.py --leg cmd).  Prints one JSON line; the full record is appended to --out (profiles/prove_enqueue.json, a list)."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"configs4": dict(m=4, t=3, nonces=False), "nonces": dict(m=1, t=3, nonces=True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=6)
    ap.add_argument("--items", type=int, default=1024)
    ap.add_argument("--shapes", default="configs4,nonces")
    ap.add_argument("--arms", default="blocking,enqueue,blocking+verify,enqueue+verify")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prove_enqueue.json"))
    ap.add_argument("--no-record", action="store_true", help="print the line, append nothing")
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    bpp = importlib.import_module("bulletproofs-plus_amd")
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    wanted = args.arms.split(",")
    stream = torch.cuda.Stream()
    run = {"tool": "bench_prove_enqueue", "items": args.items, "n_bits": 64, "reps": args.reps, "inner": args.inner,
           "box": torch.cuda.get_device_name(0), "library": os.path.basename(os.environ.get("BPP_LIB_PATH") or "") or "this tree", "shapes": []}
    with torch.cuda.stream(stream):
        eng = bpp.Engine(0, stream=stream.cuda_stream)
        n_bits, n = 64, args.items
        for name in args.shapes.split(","):
            sh = SHAPES[name]
            m, t = sh["m"], sh["t"]
            params = bpp.RangeParameters.init(n_bits, m, bpp.create_pedersen_gens_with_extension_degree(t), engine=eng)
            rounds = (n_bits * m).bit_length() - 1
            plen, need = 1 + 32 * (t + 5 + 2 * rounds), 32 * (rounds + 3)
            rng = np.random.default_rng(20261021)
            values = rng.integers(0, 1 << 63, size=(n, m), dtype=np.uint64)
            blind = rng.integers(0, 256, size=(n, m, t, 32), dtype=np.uint8)
            blind[..., 31] &= 0x0F
            minv, minp = values // np.uint64(3), np.ones((n, m), dtype=np.uint8)
            seeds = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
            seeds[:, 31] &= 0x0F
            ext = rng.integers(0, 256, size=(n, need), dtype=np.uint8)
            ms = np.full(n, m, dtype=np.uint32)
            dev = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()  # noqa: E731
            inp = packed.DeviceOpenings(dev(values), dev(blind), ms, min_values=dev(minv), min_present=dev(minp),
                                        seed_nonces=dev(seeds) if sh["nonces"] else None, rng_bytes=dev(ext), label=bench.LABEL)
            d_proofs = torch.zeros((n, plen), dtype=torch.uint8, device="cuda")
            d_commits = torch.zeros((n, 32 * m), dtype=torch.uint8, device="cuda")
            d_status = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()

            def blocking():
                res = packed.prove_openings_device(params, inp, commitments_out=d_commits, proofs_out=d_proofs, status_out=d_status)
                assert res.rc == 0, res.message
                return res

            first = blocking()
            want_proofs = d_proofs.cpu().numpy().copy()
            arms = {"blocking": blocking}
            rb = plan = None
            if any(a != "blocking" for a in wanted):
                plan = packed.ProvePlan(eng, params, ms, m_stride=m, rng_stride=need, min_values=True, min_present=True, seed_nonces=sh["nonces"],
                                        label=bench.LABEL, commit_stride=32 * m, proof_stride=plen)
                d_ok = torch.zeros((n,), dtype=torch.uint8, device="cuda")
                d_summary = torch.zeros((8,), dtype=torch.int32, device="cuda")
                d_record = torch.zeros((4,), dtype=torch.int32, device="cuda")
                outs = dict(commitments_out=d_commits, proofs_out=d_proofs, status_out=d_status, ok_mask=d_ok, summary=d_summary)

                def enqueue():
                    return plan.enqueue(inp, **outs).wait

                d_proofs.zero_()
                out = plan.enqueue(inp, **outs)
                assert out.result()["n_ok"] == n and np.array_equal(d_proofs.cpu().numpy(), want_proofs)  # (what is timed is right)
                mixed = out.as_mixed_input()
                rb = packed.ResidentBatch.from_mixed(params, first.as_mixed_input())

                def blocking_verify():
                    res = blocking()
                    fresh = packed.ResidentBatch.from_mixed(params, res.as_mixed_input())
                    fresh.verify_arrays(bpp.VerifyAction.VerifyOnly)
                    fresh.close()

                def enqueue_verify():
                    plan.enqueue(inp, **outs)
                    rb.refill(mixed, record=d_record, shape_vectors=False)
                    return rb.enqueue(chunk=0).wait

                arms.update({"enqueue": enqueue, "blocking+verify": blocking_verify, "enqueue+verify": enqueue_verify})
            arms = {k: v for k, v in arms.items() if k in wanted}

            def step(fn):
                """one step -> the wall time until its calls had returned (an enqueue arm hands back its one wait, which follows)"""
                t0 = time.perf_counter()
                wait = fn()
                t1 = time.perf_counter()
                if callable(wait):
                    wait()
                return (t1 - t0) * 1e3

            for fn in arms.values():  # warm-up: every arm, twice
                step(fn), step(fn)
            if rb is not None and "enqueue+verify" in arms:
                assert all(r["code"] == 0 for r in rb.enqueue(chunk=0).results())
            before = {"prove_enqueue": packed.prove_enqueue_stats(eng) if plan else None, "refill": packed.refill_stats(eng),
                      "enqueue": packed.enqueue_stats(eng)}
            per, cpu, calls = {k: [] for k in arms}, {k: [] for k in arms}, {k: [] for k in arms}
            for _ in range(args.reps):
                for k, fn in arms.items():
                    ts, cs, hs = [], [], []
                    for _ in range(args.inner):
                        c0, t0 = time.thread_time(), time.perf_counter()
                        hs.append(step(fn))
                        ts.append((time.perf_counter() - t0) * 1e3)
                        cs.append((time.thread_time() - c0) * 1e3)
                    per[k].append(statistics.median(ts))
                    cpu[k].append(statistics.median(cs))
                    calls[k].append(statistics.median(hs))
            row = {"shape": name, "m": m, "t": t, "nonces": sh["nonces"], "arms": {}}
            for k, v in per.items():
                med = statistics.median(v)
                row["arms"][k] = {"ms_per_step": med, "ms_low": min(v), "ms_high": max(v), "proofs_per_s": n / med * 1e3,
                                  "host_cpu_ms_per_step": statistics.median(cpu[k]), "host_ms_in_calls": statistics.median(calls[k])}
            if plan:
                after = {"prove_enqueue": packed.prove_enqueue_stats(eng), "refill": packed.refill_stats(eng), "enqueue": packed.enqueue_stats(eng)}
                row["stats_before"], row["stats_after"] = before, after
                plan.close()
                rb.close()
            run["shapes"].append(row)
            params.close()
        eng.close()
    if not args.no_record:
        runs = json.load(open(args.out)) if os.path.exists(args.out) else []
        runs.append(run)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        json.dump(runs, open(args.out, "w"), indent=1)
    print(json.dumps({"tool": "bench_prove_enqueue", "library": run["library"],
                      "ms_per_step": {r["shape"]: {k: round(a["ms_per_step"], 3) for k, a in r["arms"].items()} for r in run["shapes"]},
                      "host_ms_in_calls": {r["shape"]: {k: round(a["host_ms_in_calls"], 3) for k, a in r["arms"].items()} for r in run["shapes"]}}))


if __name__ == "__main__":
    main()
