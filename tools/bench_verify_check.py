#!/usr/bin/env python3
"""Price of a rechecked rejection ("verify_check" = 1): the same rejected call with the option off and on, one call
at a time, median wall time.

  case 1   one invalid proof (one bit of r1) in a 1024-proof call, chunk = 0: ONE group, rechecked whole
  case 2   one bad group among 64 x 1024 (chunk = 1024): passes 1 and 2 run every group's kernels, the plain MSM runs one group
  plain    bpp_msm_vartime over 16.5 k terms (the MSM of a 1024-proof group) with "msm_plain" = 0 / 1: the call's wall time,
           upload and decompression of the points included, and the kernels' registers from the built code object

One JSON line per case on stdout (profiles/verify_check_cost.jsonl is this output).  Not the headline metric: accepted calls
do not change (tools/gpu_ab.py against the parent build shows that)."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(out), min(out)


def _registers():
    try:
        txt = subprocess.run(["bash", os.path.join(ROOT, "tools", "isa", "kernel_resources.sh")], capture_output=True, text=True,
                             timeout=120).stdout
    except (OSError, subprocess.SubprocessError):
        return {}
    out = {}
    for line in txt.splitlines():
        f = line.split()
        if len(f) < 3 or "k_msm_plain" not in f[0]:
            continue
        out["k_msm_plain_sum" if "k_msm_plain_sum" in f[0] else "k_msm_plain"] = int(f[f.index("vgpr") + 1])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--groups", type=int, default=64)
    ap.add_argument("--terms", type=int, default=16500)
    args = ap.parse_args()
    bpp = importlib.import_module("bulletproofs-plus_amd")
    from tests.golden.loader import load_bench
    data = load_bench("bench_cfg2.bin")
    t = data["t"]
    eng = bpp.Engine(0)
    params = bpp.RangeParameters.init(data["bit_length"], data["m"], bpp.create_pedersen_gens_with_extension_degree(t), engine=eng)
    off_r1 = 1 + 32 * (t + 3)

    def batch(n, bad):
        its = (data["items"] * ((n + len(data["items"]) - 1) // len(data["items"])))[:n]
        sts = [bpp.RangeStatement.init(params, it["commitments"], it["min_values"], None) for it in its]
        raws = [bytes(it["proof"]) for it in its]
        raws[bad] = raws[bad][:off_r1] + bytes([raws[bad][off_r1] ^ 1]) + raws[bad][off_r1 + 1:]
        return bpp.ResidentBatch([bpp.Transcript.new(data["label"]) for _ in its], sts, [bpp.RangeProof.from_bytes(r) for r in raws])

    def rejected(rb, chunk):
        def call():
            try:
                rb.verify(bpp.VerifyAction.VerifyOnly, chunk=chunk)
            except bpp.ProofError:
                return
            raise SystemExit("the invalid batch was accepted")
        return call

    for name, n, chunk, bad in (("one invalid proof in 1024", 1024, 0, 500),
                                ("one bad group among %d x 1024" % args.groups, 1024 * args.groups, 1024, 1024 * (args.groups // 2) + 7)):
        rb = batch(n, bad)
        row = {"case": name, "proofs": n, "chunk": chunk}
        for label, v in (("unchecked", 0), ("checked", 1)):
            eng.set_option("verify_check", v)
            med, best = _timed(rejected(rb, chunk), args.iters)
            row[label + "_ms_median"], row[label + "_ms_min"] = round(med, 3), round(best, 3)
        row["stats"] = eng.verify_check_stats()
        eng.set_option("verify_check", 0)
        rb.close()
        print(json.dumps(row), flush=True)

    from oracle.pyref import curve as C
    import hashlib
    pts = [C.from_uniform_bytes(hashlib.shake_256(b"vc-p%d" % i).digest(64)).compress() for i in range(32)]
    points = [pts[i % 32] for i in range(args.terms)]
    scalars = [(int.from_bytes(hashlib.shake_256(b"vc-s%d" % i).digest(32), "little") % C.L).to_bytes(32, "little") for i in range(args.terms)]
    row = {"case": "bpp_msm_vartime", "terms": args.terms, "registers": _registers()}
    res = {}
    for label, v in (("bucket", 0), ("plain", 1)):
        eng.set_option("msm_plain", v)
        med, best = _timed(lambda: res.__setitem__(label, eng.msm_vartime(scalars, points)), args.iters)
        row[label + "_call_ms_median"], row[label + "_call_ms_min"] = round(med, 3), round(best, 3)
    eng.set_option("msm_plain", 0)
    row["equal"] = res["bucket"] == res["plain"]
    print(json.dumps(row), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
