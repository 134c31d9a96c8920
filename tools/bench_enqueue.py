#!/usr/bin/env python3
"""Stream-ordered verification (bpp_verify_enqueue) against the blocking forms, on resident inputs.

Shapes: the headline's step (64 reference batches of 1024 proofs, m = 1, 64 bits: one call with 64 groups) and a 256-proof call.
Arms, run alternately in ONE process after every arm has been warmed up on every shape:

  blocking-1        bpp_verify_resident with "chain" = 1, one call at a time, one context
  blocking-4t       the same from four threads with a context (and a resident copy of the input) each
  pipeline          packed.Pipeline: bpp_verify_submit_packed / bpp_verify_collect from host buffers, depth 4 (pays the upload too)
  enqueue-1c/2c/4c  bpp_verify_enqueue from ONE thread, four steps in flight, over 1, 2 and 4 contexts

Per (shape, arm, repetition) one JSON line: proofs/s over a window that ends in a device synchronise, the host time of the call itself
(call to return, median), process CPU seconds per step.  Before anything is timed every arm's verdicts are compared with the
blocking arm's on the same inputs, one tampered step included; a difference ends the run.  --out FILE collects the lines
(profiles/enqueue.json)."""
import argparse
import importlib
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"64x1024": (64, 1024), "1x256": (1, 256)}  # name: (groups, proofs per group)
ARMS = ("blocking-1", "blocking-4t", "pipeline", "enqueue-1c", "enqueue-2c", "enqueue-4c")
DEPTH = 4


class Slot:
    """a context with a resident copy of the good and of the tampered input"""

    def __init__(self, bpp, packed, params0, d, n, bad, chain):
        from tests.helpers import LABEL
        self.eng = bpp.Engine(0)
        if chain:
            self.eng.set_option("chain", 1)
        self.params = params0.share(self.eng)
        rest = (d["commitments"][:n], d["min_values"][:n], d["min_present"][:n], None, LABEL)
        self.good = packed.ResidentBatch(self.params, d["proofs"][:n], *rest)
        self.bad = packed.ResidentBatch(self.params, bad, *rest)

    def close(self):
        self.good.close()
        self.bad.close()
        self.params.close()
        self.eng.close()


def blocking_verdicts(packed, rb, groups, per_group):
    return [(r["code"], r["tier"], r["index"]) for r in packed.verify_groups(rb, [g * per_group for g in range(groups + 1)])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
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

    eng0 = bpp.Engine(0)
    params0 = bpp.RangeParameters.init(64, 1, bpp.create_pedersen_gens_with_extension_degree(1), engine=eng0)
    shapes = {k: v for k, v in SHAPES.items() if not args.only or k in args.only.split(",")}
    d = bench.make_inputs(np, packed, params0, max(g * p for g, p in shapes.values()), seed=20261020)
    pipe = packed.Pipeline(params0, depth=DEPTH)  # (the depth of an engine's pipeline is fixed by its first submit)
    for name, (groups, per_group) in shapes.items():
        n = groups * per_group
        bad = d["proofs"][:n].copy()
        bad[n // 2 + 7, 1 + 32 + 96 + 5] ^= 2  # one bit of r1 of one proof: its reference batch fails the final check
        slots = [Slot(bpp, packed, params0, d, n, bad, chain=True) for _ in range(4)]
        inp_good = packed.PackedInput(d["proofs"][:n], d["commitments"][:n], d["min_values"][:n], d["min_present"][:n], None, LABEL)
        inp_bad = packed.PackedInput(bad, d["commitments"][:n], d["min_values"][:n], d["min_present"][:n], None, LABEL)
        want_good = blocking_verdicts(packed, slots[0].good, groups, per_group)
        want_bad = blocking_verdicts(packed, slots[0].bad, groups, per_group)
        assert all(v == (0, 0, 0) for v in want_good) and sum(v != (0, 0, 0) for v in want_bad) == 1

        def blocking_call(slot, rb):
            try:
                rb.verify_only(per_group)
                return True
            except bpp.ProofError:
                return False

        # ---- every arm's verdicts against the blocking arm's, the tampered step included (this is also the warm-up of the shape)
        for s in slots:
            assert blocking_call(s, s.good) is True and blocking_call(s, s.bad) is False
            for rb, want in ((s.good, want_good), (s.bad, want_bad), (s.good, want_good)):
                got = [(r["code"], r["tier"], r["index"]) for r in rb.enqueue(chunk=per_group).results()]
                if got != want:
                    raise SystemExit("enqueue verdicts differ from the blocking call's: %s" % name)
        t_good, t_bad = pipe.submit(inp_good, chunk=per_group), pipe.submit(inp_bad, chunk=per_group)
        pipe.collect(t_good)
        try:
            pipe.collect(t_bad)
            raise SystemExit("pipeline accepted the tampered step: %s" % name)
        except bpp.ProofError:
            pass

        def timed(arm):
            """-> (wall seconds of `steps` steps, ended by a device synchronise; host seconds per call; CPU seconds)"""
            host = []
            torch.cuda.synchronize()
            c0, t0 = time.process_time(), time.perf_counter()
            if arm == "blocking-1":
                for _ in range(args.steps):
                    a = time.perf_counter()
                    blocking_call(slots[0], slots[0].good)
                    host.append(time.perf_counter() - a)
            elif arm == "blocking-4t":
                lock, nxt = threading.Lock(), [0]

                def worker(s):
                    while True:
                        with lock:
                            if nxt[0] >= args.steps:
                                return
                            nxt[0] += 1
                        a = time.perf_counter()
                        blocking_call(s, s.good)
                        with lock:
                            host.append(time.perf_counter() - a)
                ths = [threading.Thread(target=worker, args=(s,)) for s in slots]
                for t in ths:
                    t.start()
                for t in ths:
                    t.join()
            elif arm == "pipeline":
                flight = []
                for _ in range(args.steps):
                    if len(flight) == DEPTH:
                        pipe.collect(flight.pop(0))
                    a = time.perf_counter()
                    flight.append(pipe.submit(inp_good, chunk=per_group))
                    host.append(time.perf_counter() - a)
                for t in flight:
                    pipe.collect(t)
            else:
                k = int(arm[len("enqueue-"):-1])
                flight = []
                for i in range(args.steps):
                    if len(flight) == DEPTH:  # the depth is held by looking, with naps: a waiting thread would spin (runtime_host.h)
                        oldest = flight.pop(0)
                        while not oldest.done():
                            time.sleep(0.0002)
                    a = time.perf_counter()
                    flight.append(slots[i % k].good.enqueue(chunk=per_group, verdicts=bufs[i % DEPTH]))
                    host.append(time.perf_counter() - a)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, statistics.median(host), time.process_time() - c0

        bufs = [torch.empty((groups, 4), dtype=torch.int32, device="cuda") for _ in range(DEPTH)]
        for arm in ARMS:  # warm-up of every arm before any is timed
            saved, args.steps = args.steps, max(DEPTH, args.warmup)
            timed(arm)
            args.steps = saved
        waits0 = sum(packed.enqueue_stats(s.eng)["host_waits"] for s in slots)
        for rep in range(args.reps):
            for arm in ARMS:  # alternately
                wall, host_s, cpu = timed(arm)
                emit({"shape": name, "arm": arm, "rep": rep, "steps": args.steps, "proofs_per_step": n,
                      "proofs_per_s": round(n * args.steps / wall), "ms_per_step": round(1e3 * wall / args.steps, 4),
                      "host_ms_per_call_median": round(1e3 * host_s, 4), "cpu_s_per_step": round(cpu / args.steps, 6)})
        emit({"shape": name, "enqueue_host_waits": sum(packed.enqueue_stats(s.eng)["host_waits"] for s in slots) - waits0})
        for s in slots:
            s.close()
    params0.close()
    eng0.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
