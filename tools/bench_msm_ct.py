#!/usr/bin/env python3
"""The constant-time multiscalar multiplication of seam B1 (bpp_msm_ct_batched; csrc/ct.h: k_ct_straus<K>), timed per call: wall
time of the entry point, upload, decompression of the points and the copy back included (the call ends in a device synchronise).

  shapes      1024 groups x 2 terms (the commitment shape), 1024 x 32, 1 x 4096
  (a) forms   "msm_ct_k" = 1 against = 2 on random scalars
  (b) scalars all-zero, random, all l - 1 under the form the engine's rule takes: medians and spread side by side.  A report, not
              a pass/fail line: wall-clock equality on a shared machine proves little; the argument for uniformity is the recorded
              table reads of the host model and the shared primitives (tests/test_msm_ct_host.py)
  (c) others  bpp_msm_vartime_batched on the same inputs; for 1024 x 2 over a parameter set's exported H and G_0, bpp_pedersen_commit
  (d) build   registers, LDS and scratch of both instantiations, from the built code object (tools/isa/kernel_resources.sh)
  (e) rule    K = 1 against K = 2 alone on 512 / 768 / 2048 groups x 32 terms and 64 x 512: chunk counts on both sides of the
              form rule's threshold (csrc/ct_plan.h: ct_form_rule)

Every variant of a shape is warmed up, then the variants are timed in turn, `--reps` rounds of `--inner` calls each: a variant's
figure is the median over rounds of the round's median call, its spread the lowest and highest round.  Prints one short JSON line;
the full record goes to --out (profiles/msm_ct.json)."""
import argparse
import ctypes
import hashlib
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1024, 2), (1024, 32), (1, 4096)]
RULE_SHAPES = [(512, 32), (768, 32), (2048, 32), (64, 512)]


def _registers():
    try:
        txt = subprocess.run(["bash", os.path.join(ROOT, "tools", "isa", "kernel_resources.sh")], capture_output=True, text=True,
                             timeout=120).stdout
    except (OSError, subprocess.SubprocessError):
        return {}
    out = {}
    for line in txt.splitlines():
        f = line.split()
        if len(f) < 3 or "k_ct_straus" not in f[0]:
            continue
        name = "k_ct_straus_sum" if "straus_sum" in f[0] else ("k_ct_straus<1>" if "ILi1E" in f[0] else "k_ct_straus<2>")
        out[name] = {k: int(f[f.index(k) + 1]) for k in ("vgpr", "sgpr", "scratch", "lds")}
    return out


def _rounds(variants, reps, inner, warm=3):
    """variants: {name: callable}.  Alternating rounds -> {name: {"ms": median of rounds, "lo": .., "hi": ..}}"""
    for fn in variants.values():
        for _ in range(warm):
            fn()
    per = {k: [] for k in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            ts = []
            for _ in range(inner):
                t0 = time.perf_counter()
                fn()
                ts.append(1e3 * (time.perf_counter() - t0))
            per[name].append(statistics.median(ts))
    return {k: {"ms": round(statistics.median(v), 4), "lo": round(min(v), 4), "hi": round(max(v), 4)} for k, v in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msm_ct.json"))
    args = ap.parse_args()
    bpp = importlib.import_module("bulletproofs-plus_amd")
    from oracle.pyref import curve as C
    eng = bpp.Engine(0)
    lib, ctx = eng.lib, eng.ctx
    t_ext = 1
    params = bpp.RangeParameters.init(8, 1, bpp.create_pedersen_gens_with_extension_degree(t_ext), engine=eng)
    base_pts = [C.from_uniform_bytes(hashlib.shake_256(b"ctb-p%d" % i).digest(64)).compress() for i in range(32)]

    def check(rc):
        if rc != 0:
            raise SystemExit("engine call failed: %d" % rc)

    def ct_call(sbuf, pbuf, off, g, out):
        return lambda: check(lib.bpp_msm_ct_batched(ctx, sbuf, pbuf, off, g, out))

    def vt_call(sbuf, pbuf, off, g, out):
        return lambda: check(lib.bpp_msm_vartime_batched(ctx, sbuf, pbuf, off, g, out))

    record = {"tool": "tools/bench_msm_ct.py", "reps": args.reps, "inner": args.inner, "build": _registers(), "shapes": [], "rule_shapes": []}
    for groups, per in SHAPES + RULE_SHAPES:
        n = groups * per
        rule_only = (groups, per) in RULE_SHAPES
        commit_shape = per == 1 + t_ext
        if commit_shape:  # H and G_0 of the parameter set; the first scalar of a group is a value below 2^64
            pts = [params.h_base_compressed()] + params.g_bases_compressed()
        else:
            pts = base_pts
        pbuf = ctypes.create_string_buffer(b"".join(pts[i % len(pts)] for i in range(n)), 32 * n)
        rnd = []
        for i in range(n):
            v = int.from_bytes(hashlib.shake_256(b"ctb-s%d" % i).digest(32), "little") % C.L
            if commit_shape and i % per == 0:
                v %= 2**64
            rnd.append(v.to_bytes(32, "little"))
        scal = {"zero": bytes(32 * n), "random": b"".join(rnd), "l-1": (C.L - 1).to_bytes(32, "little") * n}
        sbuf = {k: ctypes.create_string_buffer(v, 32 * n) for k, v in scal.items()}
        off = (ctypes.c_uint32 * (groups + 1))(*[per * g for g in range(groups + 1)])
        outs = {k: ctypes.create_string_buffer(32 * groups) for k in ("ct1", "ct2", "vt", "commit")}
        row = {"groups": groups, "terms_per_group": per}

        def with_k(k, fn):
            def call():
                eng.set_option("msm_ct_k", k)
                fn()
            return call
        variants = {"ct_k1": with_k(1, ct_call(sbuf["random"], pbuf, off, groups, outs["ct1"])),
                    "ct_k2": with_k(2, ct_call(sbuf["random"], pbuf, off, groups, outs["ct2"]))}
        if rule_only:
            row["forms_and_others"] = _rounds(variants, args.reps, args.inner)
            row["equal_bytes"] = outs["ct1"].raw == outs["ct2"].raw
            eng.set_option("msm_ct_k", -1)
            record["rule_shapes"].append(row)
            continue
        variants["vartime"] = vt_call(sbuf["random"], pbuf, off, groups, outs["vt"])
        if commit_shape:
            values = (ctypes.c_uint64 * groups)(*[int.from_bytes(rnd[per * g][:8], "little") for g in range(groups)])
            blind = ctypes.create_string_buffer(b"".join(rnd[per * g + 1] for g in range(groups)), 32 * groups)
            variants["pedersen_commit"] = lambda: check(lib.bpp_pedersen_commit(ctx, params.handle, values, blind, t_ext, groups, outs["commit"]))
        row["forms_and_others"] = _rounds(variants, args.reps, args.inner)
        row["equal_bytes"] = outs["ct1"].raw == outs["ct2"].raw == outs["vt"].raw and (not commit_shape or outs["commit"].raw == outs["vt"].raw)
        eng.set_option("msm_ct_k", -1)
        row["scalar_patterns_rule_form"] = _rounds({k: ct_call(sbuf[k], pbuf, off, groups, outs["ct1"]) for k in ("zero", "random", "l-1")},
                                                   args.reps, args.inner)
        record["shapes"].append(row)
    seen, nonzero = eng.msm_ct_secret_bytes()
    record["secret_bytes"] = {"examined": seen, "nonzero": nonzero}
    params.close()
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(record) + "\n")
    short = {"bench": "msm_ct", "equal_bytes": all(r["equal_bytes"] for r in record["shapes"] + record["rule_shapes"])}
    for r in record["shapes"] + record["rule_shapes"]:
        f = r["forms_and_others"]
        short["%dx%d" % (r["groups"], r["terms_per_group"])] = {k: v["ms"] for k, v in f.items()}
    print(json.dumps(short), flush=True)


if __name__ == "__main__":
    main()
