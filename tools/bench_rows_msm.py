#!/usr/bin/env python3
"""Constant-time sums over device rows (bpp_rows_msm_enqueue) against the route a caller had before it, in one process on an engine
made on torch's stream.

Part 1, the call alone, at n = 1024 and 65 536 rows with K = 2 (shared bases and per-row points) and K = 8 (per-row points):
  device arm: calls back to back on the stream around one stream synchronise, wall time / calls (the count grows until the window is
              --window seconds)
  host-hop arm: what the parent commit offers for the same rows -- the scalars copied to the host, bpp_msm_ct_batched (k_ct_straus<1>,
              one workgroup per output; its own upload, launches, wait and download), the outputs copied to the device.  The points are
              on the host already (public, the caller's own).
  The arms alternate, --reps rounds; per arm the median of the rounds with the lowest and the highest round.  Both routes must give
  the same bytes before anything is timed.
Part 2, the commit / challenge / response step of INTEGRATION section 5 at --items rows: transcript + RNG_SCALARS -> r; R = r G;
  APPEND_POINT(X), APPEND_POINT(R), CHALLENGE_SCALAR -> c; s = c x + r.
  device      four enqueues and ONE wait
  host hops   the same step with the two host hops: r down, bpp_msm_ct_batched, R up; c and r down, Python integers, s up
No figure is asserted: a record, not a gate.  Prints one JSON line; the record goes to --out (profiles/rows_msm.json)."""
import argparse
import ctypes
import hashlib
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,65536")
    ap.add_argument("--window", type=float, default=0.5, help="seconds of device calls per timed window")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--items", type=int, default=1024)
    ap.add_argument("--inner", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_msm.json"))
    ap.add_argument("--no-record", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from oracle.pyref import curve as C
    bpp = importlib.import_module("bulletproofs-plus_amd")
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    stream = torch.cuda.Stream()
    L = C.L
    rec = {"tool": "bench_rows_msm", "box": torch.cuda.get_device_name(0), "window_s": args.window, "reps": args.reps, "cases": [], "step": None}
    pool = np.stack([np.frombuffer(C.from_uniform_bytes(hashlib.shake_256(b"bench-rows-%d" % i).digest(64)).compress(), dtype=np.uint8)
                     for i in range(32)])
    with torch.cuda.stream(stream):
        eng = bpp.Engine(0, stream=stream.cuda_stream)
        lib = eng.lib

        def window(fn):
            k = 4
            while True:
                stream.synchronize()
                t0 = time.perf_counter()
                for _ in range(k):
                    fn()
                stream.synchronize()
                dt = time.perf_counter() - t0
                if dt >= args.window or k >= (1 << 15):
                    return dt / k * 1e3, k
                k = min(k * max(2, int(args.window / max(dt, 1e-4)) + 1), 1 << 15)

        def host_msm(sc_dev, pt_host, K, out_dev):
            """the parent commit's route: scalars down, bpp_msm_ct_batched, outputs up"""
            sc = sc_dev.cpu().numpy()
            n = sc.shape[0]
            goff = np.arange(0, K * (n + 1), K, dtype=np.uint32)
            out = np.zeros((n, 32), dtype=np.uint8)
            rc = lib.bpp_msm_ct_batched(eng.ctx, sc.ctypes.data, pt_host.ctypes.data, goff.ctypes.data, n, out.ctypes.data)
            assert rc == 0, rc
            out_dev.copy_(torch.from_numpy(out))
            torch.cuda.current_stream().synchronize()

        def canonical(rng, shape):
            a = rng.integers(0, 256, size=shape + (32,), dtype=np.uint8)
            a[..., 31] &= 0x0F
            return a

        # ---- part 1
        for n in [int(x) for x in args.sizes.split(",")]:
            for name, K, shared in (("K2_shared", 2, True), ("K2_rows", 2, False), ("K8_rows", 8, False)):
                rng = np.random.default_rng(1000 * K + n + shared)
                sc = torch.from_numpy(canonical(rng, (n, K)).reshape(n, 32 * K)).cuda()
                idx = rng.integers(0, 32, size=(1 if shared else n, K))
                pt_rows = pool[idx].reshape(-1, 32 * K)
                pt_host = np.ascontiguousarray(np.broadcast_to(pt_rows, (n, 32 * K)))  # the host route has no shared form
                pt = torch.from_numpy(pt_rows.reshape(K, 32) if shared else pt_rows).cuda()
                out, out_host = torch.zeros((n, 32), dtype=torch.uint8, device="cuda"), torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
                done, record = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
                dev_fn = lambda: packed.rows_msm(eng, sc, pt, K, out=out, done_mask=done, record=record)  # noqa: E731
                host_fn = lambda: host_msm(sc, pt_host, K, out_host)  # noqa: E731
                dev_fn().wait()
                host_fn()
                assert torch.equal(out, out_host), "%s n=%d: the device rows differ from the host route's" % (name, n)
                assert int(record.cpu()[0]) == n
                dev_fn(), host_fn()
                dv, hs, calls = [], [], 0
                for _ in range(args.reps):
                    ms, calls = window(dev_fn)
                    dv.append(ms)
                    t0 = time.perf_counter()
                    host_fn()
                    hs.append((time.perf_counter() - t0) * 1e3)
                d, h = statistics.median(dv), statistics.median(hs)
                rec["cases"].append({"case": name, "n": n, "K": K, "shared": shared, "device_ms_per_call": d, "device_ms_low": min(dv),
                                     "device_ms_high": max(dv), "device_calls_in_window": calls, "device_us_per_output": d / n * 1e3,
                                     "device_outputs_per_s": n / d * 1e3, "host_hop_ms_per_step": h, "host_hop_ms_low": min(hs),
                                     "host_hop_ms_high": max(hs), "host_hop_us_per_output": h / n * 1e3, "host_hop_over_device": h / d})

        # ---- part 2
        n = args.items
        rng = np.random.default_rng(20261021)
        x_np = canonical(rng, (n,))
        x_int = [int.from_bytes(bytes(r), "little") for r in x_np]
        G = np.frombuffer(C.BASEPOINT.compress(), dtype=np.uint8).copy()
        G_rows = np.ascontiguousarray(np.broadcast_to(G, (n, 32)))
        d_x, d_G = torch.from_numpy(x_np).cuda(), torch.from_numpy(G.reshape(1, 32)).cuda()
        d_X = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
        packed.rows_msm(eng, d_x, d_G, 1, out=d_X).wait()  # X = x G
        txid = torch.from_numpy(rng.integers(0, 256, size=(n, 32), dtype=np.uint8)).cuda()
        rows = torch.zeros((n, 203), dtype=torch.uint8, device="cuda")
        r, R, c, s = (torch.zeros((n, 32), dtype=torch.uint8, device="cuda") for _ in range(4))
        done1, done2, done3 = (torch.zeros(n, dtype=torch.uint8, device="cuda") for _ in range(3))
        rec1, rec2, rec3 = (torch.zeros(4, dtype=torch.int32, device="cuda") for _ in range(3))
        ops1 = [packed.TNew(b"bench rows step"), packed.TAppend(b"txid", txid), packed.TRngBegin(), packed.TRngRekey(b"x", d_x),
                packed.TRngFinalize(None), packed.TRngScalars(1, r)]
        ops2 = [packed.TAppendPoint(b"X", d_X), packed.TAppendPoint(b"R", R), packed.TChallengeScalar(b"c", c)]

        def step_device():
            packed.transcript_ops(eng, rows, ops1, done_mask=done1, record=rec1)
            packed.rows_msm(eng, r, d_G, 1, out=R, done_mask=done3, record=rec3)
            packed.transcript_ops(eng, rows, ops2, done_mask=done2, record=rec2)
            packed.rows_scalar_muladd(eng, c, d_x, r, out=s, live=done2, done_mask=done3, record=rec3).wait()

        def step_host():
            packed.transcript_ops(eng, rows, ops1, done_mask=done1, record=rec1)
            host_msm(r, G_rows, 1, R)
            packed.transcript_ops(eng, rows, ops2, done_mask=done2, record=rec2).wait()
            ch, rh = c.cpu().numpy(), r.cpu().numpy()
            sh = np.zeros((n, 32), dtype=np.uint8)
            for i in range(n):
                v = (int.from_bytes(bytes(ch[i]), "little") * x_int[i] + int.from_bytes(bytes(rh[i]), "little")) % L
                sh[i] = np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint8)
            s.copy_(torch.from_numpy(sh))
            torch.cuda.current_stream().synchronize()

        step_device()
        want = (rows.clone(), R.clone(), c.clone(), s.clone())
        assert int(rec3.cpu()[0]) == n, "the device step left rows undone"
        step_host()
        assert all(torch.equal(a, b) for a, b in zip(want, (rows, R, c, s))), "the two steps differ"
        arms = {"device": step_device, "host_hops": step_host}
        for fn in arms.values():
            fn()
        per = {k: [] for k in arms}
        for _ in range(args.reps):
            for k, fn in arms.items():
                ts = []
                for _ in range(args.inner):
                    t0 = time.perf_counter()
                    fn()
                    ts.append((time.perf_counter() - t0) * 1e3)
                per[k].append(statistics.median(ts))
        step = {"items": n, "reps": args.reps, "inner": args.inner, "arms": {}}
        for k, v in per.items():
            med = statistics.median(v)
            step["arms"][k] = {"ms_per_step": med, "ms_low": min(v), "ms_high": max(v), "rows_per_s": n / med * 1e3}
        step["host_hops_over_device"] = step["arms"]["host_hops"]["ms_per_step"] / step["arms"]["device"]["ms_per_step"]
        step["stats"] = {"rows": packed.rows_stats(eng), "transcripts": packed.transcripts_stats(eng)}
        rec["step"] = step
        eng.close()
    if not args.no_record:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        json.dump(rec, open(args.out, "w"), indent=1)
    print(json.dumps({"tool": "bench_rows_msm",
                      "device_us_per_output": {"%s@%d" % (r["case"], r["n"]): round(r["device_us_per_output"], 3) for r in rec["cases"]},
                      "host_hop_over_device": {"%s@%d" % (r["case"], r["n"]): round(r["host_hop_over_device"], 2) for r in rec["cases"]},
                      "step_ms": {k: [round(a["ms_low"], 3), round(a["ms_per_step"], 3), round(a["ms_high"], 3)] for k, a in rec["step"]["arms"].items()}}))


if __name__ == "__main__":
    main()
