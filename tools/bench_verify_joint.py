#!/usr/bin/env python3
"""The joint final check ("verify_joint" = 1) against the per-group MSMs: resident inputs, several steps in flight the
way bench.py's headline leg runs them (one context and one resident copy of the input per slot), proofs/s and ms per call with
the option off (0) and the joint form forced (2: with 1 the engine's rule leaves groups above 14 000 terms on the per-group path,
which is what these figures are the reason for).

  64x1024      64 reference batches of 1024 proofs (m = 1, 64 bits): the headline's step
  16x256       the batcher's pooled shape
  4x1024-m8    aggregated proofs, m = 8
  64x1024-bad  the first shape with one invalid proof (one bit of r1): the price of a fall-back
  16x16, 8x2   small pooled calls, for the term count up to which the joint form is taken

For the first shape also the joint plan (bpp_msm_last_plan) and the prelude's event time (bpp_profile: msm_sort_ms) of the joint
MSM with the one-workgroup form ("msm_prelude_slices" = 1) against the sliced one (the engine's rule, and --slices).

One JSON line per (shape, arm) on stdout; --out FILE collects them (profiles/verify_joint.json is this output next to the
tools/gpu_ab.py run against the parent build).  --only NAME[,NAME] runs those shapes; --arms 0,2 chooses the option's values; BPP_LIB_PATH
names another build of the library (only arm 0 exists in a build without the option)."""
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

SHAPES = {  # name: (groups, proofs per group, aggregation, invalid proof or None)
    "64x1024": (64, 1024, 1, None),
    "16x256": (16, 256, 1, None),
    "4x1024-m8": (4, 1024, 8, None),
    "64x1024-bad": (64, 1024, 1, 32 * 1024 + 7),
    # small pooled calls (a batcher's callers with a few proofs each): where the rule's term bound comes from
    "16x16": (16, 16, 1, None),
    "8x2": (8, 2, 1, None),
}


def run_leg(bpp, packed, np, params0, d, groups, per_group, bad, options, slots, steps, warmup, profile=False):
    """`steps` timed calls over `slots` slots in flight; returns (seconds, latencies, engines' stats, last plan, stage profiles)"""
    from tests.helpers import LABEL
    n = groups * per_group
    proofs = d["proofs"][:n]
    if bad is not None:
        proofs = proofs.copy()
        proofs[bad, 1 + 32 + 96 + 5] ^= 2
    made = []
    for _ in range(slots):
        eng = bpp.Engine(0)
        for k, v in options.items():
            eng.set_option(k, v)
        eng.profile(1 if profile else 0)
        params = params0.share(eng)
        rb = packed.ResidentBatch(params, proofs, d["commitments"][:n], d["min_values"][:n], d["min_present"][:n], None, LABEL)
        rb.prepare(per_group)
        made.append((eng, params, rb))

    def call(rb):
        try:
            rb.verify_only(per_group)
            ok = True
        except bpp.ProofError:
            ok = False
        if ok != (bad is None):
            raise SystemExit("wrong verdict: %s" % ("accepted an invalid input" if ok else "rejected a valid input"))

    for _, _, rb in made:
        for _ in range(max(1, warmup)):
            call(rb)
    lat, profs, lock, nxt, errors = [], [], threading.Lock(), [0], []

    def worker(slot):
        eng, _, rb = made[slot]
        try:
            while True:
                with lock:
                    if nxt[0] >= steps or errors:
                        return
                    nxt[0] += 1
                t0 = time.perf_counter()
                call(rb)
                dt = time.perf_counter() - t0
                with lock:
                    lat.append(dt)
                    if profile:
                        profs.append(eng.last_profile())
        except BaseException as e:  # noqa: BLE001 - re-raised on the calling thread
            with lock:
                errors.append(e)
    ths = [threading.Thread(target=worker, args=(s,)) for s in range(slots)]
    t0 = time.perf_counter()
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    wall = time.perf_counter() - t0
    if errors:
        raise errors[0]
    stats = None
    if hasattr(made[0][0], "verify_joint_stats") and hasattr(made[0][0].lib, "bpp_verify_joint_stats"):
        stats = {}
        for eng, _, _ in made:
            for k, v in eng.verify_joint_stats().items():
                stats[k] = stats.get(k, 0) + v
    plan = made[0][0].msm_last_plan()
    for eng, params, rb in made:
        rb.close()
        params.close()
        eng.close()
    return wall, lat, stats, plan, profs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--slots", type=int, default=4)
    ap.add_argument("--only", default="")
    ap.add_argument("--arms", default="0,2")
    ap.add_argument("--slices", default="", help="extra slice counts for the prelude comparison, e.g. 16,32,64")
    ap.add_argument("--no-prelude", action="store_true", help="skip the prelude comparison")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import bench
    bpp = importlib.import_module("bulletproofs-plus_amd")
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    arms = [int(x) for x in args.arms.split(",") if x != ""]
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    eng0 = bpp.Engine(0)
    data = {}
    for name, (groups, per_group, m, bad) in SHAPES.items():
        if args.only and name not in args.only.split(","):
            continue
        if m not in data:
            params0 = bpp.RangeParameters.init(64, m, bpp.create_pedersen_gens_with_extension_degree(1), engine=eng0)
            need = max(g * p for g, p, mm, _ in SHAPES.values() if mm == m)
            data[m] = (params0, bench.make_inputs(np, packed, params0, need, seed=20261019 + m))
        params0, d = data[m]
        for joint in arms:
            wall, lat, stats, plan, _ = run_leg(bpp, packed, np, params0, d, groups, per_group, bad, {"verify_joint": joint} if joint else {},
                                                args.slots, args.steps, args.warmup)
            emit({"shape": name, "verify_joint": joint, "proofs": groups * per_group, "slots": args.slots, "steps": args.steps,
                  "proofs_per_s": round(groups * per_group * args.steps / wall), "ms_per_call": round(1e3 * wall / args.steps, 4),
                  "latency_ms_median": round(1e3 * statistics.median(lat), 4), "joint_stats": stats,
                  "last_plan": {k: plan[k] for k in ("c", "K", "nb", "G", "terms", "quad", "reduce", "form", "dig_cap")}})
        if name == "64x1024" and 2 in arms and not args.no_prelude:
            # the joint MSM's prelude alone, one call at a time with stage events: one-workgroup form, the rule's slices, others
            for label, s in [("one-workgroup", 1), ("rule", 0)] + [("S=%s" % x, int(x)) for x in args.slices.split(",") if x]:
                _, lat, _, plan, profs = run_leg(bpp, packed, np, params0, d, groups, per_group, None,
                                                 {"verify_joint": 2, "msm_prelude_slices": s}, 1, 8, 2, profile=True)
                emit({"shape": name, "prelude": label, "slices": (plan["form"] >> 8) & 0xff, "c": plan["c"], "terms": plan["terms"],
                      "prelude_ms_median": round(statistics.median(p["msm_sort_ms"] for p in profs), 4),
                      "accumulate_ms_median": round(statistics.median(p["msm_accumulate_ms"] for p in profs), 4),
                      "bucket_reduce_ms_median": round(statistics.median(p["msm_bucket_reduce_ms"] for p in profs), 4),
                      "call_ms_median": round(1e3 * statistics.median(lat), 4)})
    for params0, _ in data.values():
        params0.close()
    eng0.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
