#!/usr/bin/env python3
"""Merlin on the stream (bpp_transcripts_enqueue) against the host route, in one process on an engine made on torch's stream.

Part 1, the call alone, at n = 1024 and 65 536 rows:
  make        NEW(label) + APPEND("txid", 32 bytes per row): the rows a *_transcripts call takes
  challenge   CHALLENGE("next", 32) on rows that are transcripts: going on with the rows a *_states call hands back
  device arm: K calls on the stream, one stream synchronise, wall time / K (K grows until the window is --window seconds)
  host arm:   what a caller without the call does per step -- copy the rows (or the transaction ids) down, run
              bpp_transcript_new / bpp_transcript_append_message / bpp_transcript_challenge_bytes per row, copy the result up.
              From Python every helper call goes through ctypes; the record carries the measured cost of as many empty ctypes calls
              (`ctypes_overhead_ms`) so that a reader can take it off: `host_ms_less_ctypes` is what a compiled caller would see.
Part 2, the full step of INTEGRATION section 5 ("Proving on the stream") at --items proofs (m = 1, t = 1, 64 bits):
  device      make the rows on the device -> plan.enqueue -> refill -> verify enqueue (states) -> CHALLENGE on the rows: ONE wait
  host        the same step with the host route at both ends: the rows made on the host and copied up; the step's one wait; the
              advanced rows copied down, challenged on the host, the challenges copied up
  The arms alternate; per arm the median over --reps rounds of the round's median step, with the lowest and highest round (the spread).
No figure is asserted: a record, not a gate.  Prints one JSON line; the record goes to --out (profiles/transcript_ops.json)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,65536")
    ap.add_argument("--window", type=float, default=1.5, help="seconds of device calls per timed window")
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--items", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transcript_ops.json"))
    ap.add_argument("--no-record", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    bpp = importlib.import_module("bulletproofs-plus_amd")
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    stream = torch.cuda.Stream()
    rec = {"tool": "bench_transcript_ops", "box": torch.cuda.get_device_name(0), "window_s": args.window, "sizes": [], "full_step": None}
    label, l_txid, l_next = b"bench transcript ops", b"txid", b"next"
    u8 = lambda b: (ctypes.c_uint8 * len(b)).from_buffer_copy(b)  # noqa: E731
    c_label, c_txid, c_next = u8(label), u8(l_txid), u8(l_next)
    with torch.cuda.stream(stream):
        eng = bpp.Engine(0, stream=stream.cuda_stream)
        lib = eng.lib

        def host_make(txid_dev, rows_dev):
            """the host route of `make`: ids down, new + append per row, rows up"""
            txid = txid_dev.cpu().numpy()
            n = txid.shape[0]
            rows = np.zeros((n, 203), dtype=np.uint8)
            base, tbase = rows.ctypes.data, txid.ctypes.data
            for i in range(n):
                lib.bpp_transcript_new(c_label, len(label), base + 203 * i)
                lib.bpp_transcript_append_message(base + 203 * i, c_txid, len(l_txid), tbase + 32 * i, 32)
            rows_dev.copy_(torch.from_numpy(rows))
            torch.cuda.current_stream().synchronize()

        def host_challenge(rows_dev, out_dev):
            """the host route of `challenge`: rows down, challenge per row, rows and challenges up"""
            rows = rows_dev.cpu().numpy()
            n = rows.shape[0]
            out = np.zeros((n, 32), dtype=np.uint8)
            base, obase = rows.ctypes.data, out.ctypes.data
            for i in range(n):
                if rows[i, 202]:  # (a zero row is no transcript: it stays zero, as on the device)
                    lib.bpp_transcript_challenge_bytes(base + 203 * i, c_next, len(l_next), obase + 32 * i, 32)
            rows_dev.copy_(torch.from_numpy(rows))
            out_dev.copy_(torch.from_numpy(out))
            torch.cuda.current_stream().synchronize()

        def ctypes_overhead(calls):
            """the lowest of four passes of `calls` empty ctypes calls (the first pass warms the path)"""
            best = None
            for _ in range(4):
                t0 = time.perf_counter()
                for _ in range(calls):
                    lib.bpp_host_threads()
                dt = (time.perf_counter() - t0) * 1e3
                best = dt if best is None else min(best, dt)
            return best

        def window(fn):
            """K calls and one synchronise; K doubles until the window is long enough -> ms per call, K"""
            k = 8
            while True:
                stream.synchronize()
                t0 = time.perf_counter()
                for _ in range(k):
                    fn()
                stream.synchronize()
                dt = time.perf_counter() - t0
                if dt >= args.window or k >= (1 << 17):
                    return dt / k * 1e3, k
                k = min(k * max(2, int(args.window / max(dt, 1e-4)) + 1), 1 << 17)

        # ---- part 1
        for n in [int(x) for x in args.sizes.split(",")]:
            rng = np.random.default_rng(n)
            txid = torch.from_numpy(rng.integers(0, 256, size=(n, 32), dtype=np.uint8)).cuda()
            rows = torch.full((n, 203), 0xFF, dtype=torch.uint8, device="cuda")
            rows_host = torch.zeros((n, 203), dtype=torch.uint8, device="cuda")
            out = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
            out_host = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
            done, record = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
            make_ops = [packed.TNew(label), packed.TAppend(l_txid, txid)]
            chal_ops = [packed.TChallenge(l_next, 32, out)]
            make = lambda: packed.transcript_ops(eng, rows, make_ops, done_mask=done, record=record)  # noqa: E731
            chal = lambda: packed.transcript_ops(eng, rows, chal_ops, done_mask=done, record=record)  # noqa: E731
            # what is timed is right: both routes give the same bytes
            make().wait()
            host_make(txid, rows_host)
            assert torch.equal(rows, rows_host), "make: the device rows differ from the host route's"
            chal().wait()
            host_challenge(rows_host, out_host)
            assert torch.equal(rows, rows_host) and torch.equal(out, out_host), "challenge: the device differs from the host route"
            row = {"n": n, "arms": {}}
            for name, dev_fn, host_fn, calls in (("make", make, lambda: host_make(txid, rows_host), 2 * n),
                                                 ("challenge", chal, lambda: host_challenge(rows_host, out_host), n)):
                dev_fn(), dev_fn()
                dev_ms, k = window(dev_fn)
                host_fn()
                hs = []
                for _ in range(args.host_steps if n > 4096 else 8 * args.host_steps):
                    t0 = time.perf_counter()
                    host_fn()
                    hs.append((time.perf_counter() - t0) * 1e3)
                host_ms, over = statistics.median(hs), ctypes_overhead(calls)
                row["arms"][name] = {"device_ms_per_call": dev_ms, "device_calls_in_window": k, "device_rows_per_s": n / dev_ms * 1e3,
                                     "host_ms_per_step": host_ms, "host_ms_low": min(hs), "host_ms_high": max(hs), "ctypes_overhead_ms": over,
                                     "host_ms_less_ctypes": host_ms - over, "host_over_device": host_ms / dev_ms,
                                     "host_less_ctypes_over_device": (host_ms - over) / dev_ms}
            row["stats"] = packed.transcripts_stats(eng)
            rec["sizes"].append(row)

        # ---- part 2
        n, n_bits, m, t = args.items, 64, 1, 1
        params = bpp.RangeParameters.init(n_bits, m, bpp.create_pedersen_gens_with_extension_degree(t), engine=eng)
        rounds = (n_bits * m).bit_length() - 1
        need = 32 * (rounds + 3)
        rng = np.random.default_rng(20261021)
        dev = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()  # noqa: E731
        values = rng.integers(0, 1 << 63, size=(n, m), dtype=np.uint64)
        blind = rng.integers(0, 256, size=(n, m, t, 32), dtype=np.uint8)
        blind[..., 31] &= 0x0F
        ext = rng.integers(0, 256, size=(n, need), dtype=np.uint8)
        ms = np.full(n, m, dtype=np.uint32)
        txid = dev(rng.integers(0, 256, size=(n, 32), dtype=np.uint8))
        rows = torch.full((n, 203), 0xFF, dtype=torch.uint8, device="cuda")
        nxt = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
        done, record = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
        make_ops = [packed.TNew(label), packed.TAppend(l_txid, txid)]
        plan = packed.ProvePlan(eng, params, ms, m_stride=m, rng_stride=need, item_states=True)
        inp = packed.DeviceOpenings(dev(values), dev(blind), ms, rng_bytes=dev(ext), item_states=rows)
        outs = dict(commitments_out=torch.zeros((n, 32 * m), dtype=torch.uint8, device="cuda"),
                    proofs_out=torch.zeros((n, plan.proof_stride), dtype=torch.uint8, device="cuda"),
                    status_out=torch.zeros((n, 2), dtype=torch.int32, device="cuda"), ok_mask=torch.zeros(n, dtype=torch.uint8, device="cuda"),
                    summary=torch.zeros(8, dtype=torch.int32, device="cuda"), states=torch.zeros((n, 203), dtype=torch.uint8, device="cuda"))
        verified = torch.zeros((n, 203), dtype=torch.uint8, device="cuda")
        refill_rec = torch.zeros(4, dtype=torch.int32, device="cuda")
        packed.transcript_ops(eng, rows, make_ops, done_mask=done, record=record)
        first = plan.enqueue(inp, **outs)
        assert first.result()["n_ok"] == n
        mixed = first.as_mixed_input()
        rb = packed.ResidentBatch.from_mixed(params, mixed)
        rb.enqueue(chunk=0, states=verified).wait()

        def step_device():
            packed.transcript_ops(eng, rows, make_ops, done_mask=done, record=record)
            plan.enqueue(inp, **outs)
            rb.refill(mixed, record=refill_rec, shape_vectors=False)
            rb.enqueue(chunk=0, states=verified)
            packed.transcript_ops(eng, verified, [packed.TChallenge(l_next, 32, nxt)], done_mask=done, record=record).wait()

        def step_host():
            host_make(txid, rows)
            plan.enqueue(inp, **outs)
            rb.refill(mixed, record=refill_rec, shape_vectors=False)
            rb.enqueue(chunk=0, states=verified).wait()
            host_challenge(verified, nxt)

        step_device()
        want = (verified.clone(), nxt.clone())
        assert int(record.cpu()[0]) == n, "the device step left rows undone"
        step_host()
        assert torch.equal(verified, want[0]) and torch.equal(nxt, want[1]), "the two steps differ"
        arms = {"device": step_device, "host": step_host}
        for fn in arms.values():
            fn(), fn()
        per = {k: [] for k in arms}
        for _ in range(args.reps):
            for k, fn in arms.items():
                ts = []
                for _ in range(args.inner):
                    t0 = time.perf_counter()
                    fn()
                    ts.append((time.perf_counter() - t0) * 1e3)
                per[k].append(statistics.median(ts))
        full = {"items": n, "n_bits": n_bits, "m": m, "t": t, "reps": args.reps, "inner": args.inner, "arms": {}}
        for k, v in per.items():
            med = statistics.median(v)
            full["arms"][k] = {"ms_per_step": med, "ms_low": min(v), "ms_high": max(v), "rounds": v, "proofs_per_s": n / med * 1e3}
        full["host_over_device"] = full["arms"]["host"]["ms_per_step"] / full["arms"]["device"]["ms_per_step"]
        full["ctypes_overhead_ms"] = ctypes_overhead(3 * n)
        full["stats"] = {"transcripts": packed.transcripts_stats(eng), "prove_enqueue": packed.prove_enqueue_stats(eng),
                         "refill": packed.refill_stats(eng), "enqueue": packed.enqueue_stats(eng)}
        rec["full_step"] = full
        plan.close()
        rb.close()
        params.close()
        eng.close()
    if not args.no_record:
        old = json.load(open(args.out)) if os.path.exists(args.out) else {}
        if "bench_ab" in old:
            rec["bench_ab"] = old["bench_ab"]  # (tools/gpu_ab.py's lines of the headline against the parent commit: kept)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        json.dump(rec, open(args.out, "w"), indent=1)
    print(json.dumps({"tool": "bench_transcript_ops",
                      "host_over_device": {str(r["n"]): {k: round(a["host_over_device"], 2) for k, a in r["arms"].items()} for r in rec["sizes"]},
                      "device_ms_per_call": {str(r["n"]): {k: round(a["device_ms_per_call"], 4) for k, a in r["arms"].items()} for r in rec["sizes"]},
                      "full_step_ms": {k: [round(a["ms_low"], 3), round(a["ms_per_step"], 3), round(a["ms_high"], 3)] for k, a in rec["full_step"]["arms"].items()}}))


if __name__ == "__main__":
    main()
