#!/usr/bin/env python3
"""Proving from openings in device memory against proving from host arrays, timed per call:

  host    bpp_prove_openings over a bpp_prove_item array whose rows lie in host memory (ProvePack, page-locked staging, uploads,
          proofs and commitments back through page-locked staging) -- the existing form, the baseline, not code under test
  device  bpp_prove_openings_device over the same rows resident in device memory (csrc/prove_ingest.h: k_prove_ingest, k_prove_emit);
          proofs and commitments stay on the device

and, as a third figure per arm, the prove call FOLLOWED by a mixed upload of what it wrote: host prove + bpp_batch_upload_mixed
from the host rows against device prove + bpp_batch_upload_mixed_device of the device rows (each upload followed by
bpp_batch_destroy inside the timed span).  Two shapes: configs[4] (1024 x m = 4, t = 3, 64 bits) and 1024 x m = 1, t = 3, a seed
nonce on each.  The arms alternate in one process, both warmed up, then `--reps` rounds of `--inner` calls each; per arm the median
over rounds of the round's median wall time per call with the lowest and highest round.  A record, not a gate: no ratio is asserted
anywhere and no rate is promised -- the prover is bound by its instruction rate, and the copies the device form removes are a few
hundred microseconds of a call of several milliseconds.  Prints one short JSON line; the full record is appended to --out
(profiles/prove_device.json, a list of runs).

--item-states: another pair of arms instead, configs[4]'s shape only -- bpp_prove_openings_device_transcripts with one transcript row
per item going in and the advanced rows coming out (k_prove_item_states in front of kp_init, kp_finish<true>, the rows through
k_prove_emit) against bpp_prove_openings_device on the same openings under one label, alternating in the same way; the record goes to
profiles/prove_device_states.json.  The rows add about three cooperative permutations per proof in front of the call."""
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

SHAPES = {"configs4": dict(m=4, t=3, nonces=False), "nonces": dict(m=1, t=3, nonces=True)}


def item_states_arms(args):
    import numpy as np
    import torch
    import bench
    bpp = importlib.import_module("bulletproofs-plus_amd")
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    eng = bpp.Engine(0)
    n_bits, n, m, t = 64, args.items, SHAPES["configs4"]["m"], SHAPES["configs4"]["t"]
    params = bpp.RangeParameters.init(n_bits, m, bpp.create_pedersen_gens_with_extension_degree(t), engine=eng)
    rounds = (n_bits * m).bit_length() - 1
    plen, need = 1 + 32 * (t + 5 + 2 * rounds), 32 * (rounds + 3)
    rng = np.random.default_rng(20261021)
    values = rng.integers(0, 1 << 63, size=(n, m), dtype=np.uint64)
    blind = rng.integers(0, 256, size=(n, m, t, 32), dtype=np.uint8)
    blind[..., 31] &= 0x0F
    minv, minp = values // np.uint64(3), np.ones((n, m), dtype=np.uint8)
    ext = rng.integers(0, 256, size=(n, need), dtype=np.uint8)
    ms = np.full(n, m, dtype=np.uint32)
    # one transcript per item: the label, then a context whose length differs from item to item (so do the rows' positions)
    rows = np.zeros((n, 203), dtype=np.uint8)
    for i in range(n):
        tr = bpp.Transcript.new(bench.LABEL)
        tr.append_message(b"ctx", bytes([i & 255]) * (1 + i % 167))
        rows[i] = np.frombuffer(tr.state, dtype=np.uint8)
    dev = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()  # noqa: E731
    arrays = dict(min_values=dev(minv), min_present=dev(minp), rng_bytes=dev(ext))
    plain = packed.DeviceOpenings(dev(values), dev(blind), ms, label=bench.LABEL, **arrays)
    with_rows = packed.DeviceOpenings(dev(values), dev(blind), ms, item_states=dev(rows), **arrays)
    d_proofs = torch.zeros((n, plen), dtype=torch.uint8, device="cuda")
    d_commits = torch.zeros((n, 32 * m), dtype=torch.uint8, device="cuda")
    d_status = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    d_states = torch.zeros((n, 203), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def call(inp, states):
        res = packed.prove_openings_device(params, inp, commitments_out=d_commits, proofs_out=d_proofs, status_out=d_status, states=states)
        assert res.rc == 0, res.message
        return res

    arms = {"device": lambda: call(plain, None), "device+item_states": lambda: call(with_rows, d_states)}
    res = arms["device+item_states"]()
    packed.verify_batch_mixed_device(params, res.as_mixed_input())  # (what is timed is right: the outputs verify under their own rows)
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
    run = {"tool": "bench_prove_device --item-states", "items": n, "n_bits": n_bits, "m": m, "t": t, "reps": args.reps, "inner": args.inner,
           "box": torch.cuda.get_device_name(0), "arms": {}}
    for k, v in per.items():
        med = statistics.median(v)
        run["arms"][k] = {"ms_per_call": med, "ms_low": min(v), "ms_high": max(v), "proofs_per_s": n / med * 1e3}
    run["stats"] = packed.prove_device_stats(eng)
    runs = json.load(open(args.out)) if os.path.exists(args.out) else []
    runs.append(run)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(runs, open(args.out, "w"), indent=1)
    print(json.dumps({"tool": run["tool"], "ms_per_call": {k: round(a["ms_per_call"], 3) for k, a in run["arms"].items()}}))
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=6)
    ap.add_argument("--items", type=int, default=1024)
    ap.add_argument("--shapes", default="configs4,nonces")
    ap.add_argument("--out", default=None)
    ap.add_argument("--item-states", action="store_true", help="time per-item transcripts in and out against the call without them")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "prove_device_states.json" if args.item_states else "prove_device.json")
    if args.item_states:
        return item_states_arms(args)
    import numpy as np
    import torch
    import bench
    bpp = importlib.import_module("bulletproofs-plus_amd")
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    lib_mod = importlib.import_module("bulletproofs-plus_amd._lib")
    eng = bpp.Engine(0)
    lib = eng.lib
    n_bits, n = 64, args.items
    run = {"tool": "bench_prove_device", "items": n, "n_bits": n_bits, "reps": args.reps, "inner": args.inner,
           "box": torch.cuda.get_device_name(0), "shapes": []}
    for name in args.shapes.split(","):
        sh = SHAPES[name]
        m, t = sh["m"], sh["t"]
        params = bpp.RangeParameters.init(n_bits, m, bpp.create_pedersen_gens_with_extension_degree(t), engine=eng)
        rounds = (n_bits * m).bit_length() - 1
        plen, need = 1 + 32 * (t + 5 + 2 * rounds), 32 * (rounds + 3)
        rng = np.random.default_rng(20261020)
        values = rng.integers(0, 1 << 63, size=(n, m), dtype=np.uint64)
        blind = rng.integers(0, 256, size=(n, m, t, 32), dtype=np.uint8)
        blind[..., 31] &= 0x0F
        minv, minp = values // np.uint64(3), np.ones((n, m), dtype=np.uint8)
        seeds = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        seeds[:, 31] &= 0x0F
        ext = rng.integers(0, 256, size=(n, need), dtype=np.uint8)
        ms = np.full(n, m, dtype=np.uint32)
        # host arm: the item array over the host rows, outputs in host memory
        items = np.zeros(n, dtype=packed._PROVE_ITEM)
        items["values"], items["blindings32"], items["m"] = packed._rows(values), packed._rows(blind), m
        items["min_values"], items["min_present"] = packed._rows(minv), packed._rows(minp)
        if sh["nonces"]:
            items["seed_nonce32"] = packed._rows(seeds)
        label = np.frombuffer(bench.LABEL, dtype=np.uint8).copy()
        items["transcript_label"], items["label_len"] = label.ctypes.data, len(bench.LABEL)
        items["rng_bytes"], items["rng_len"] = packed._rows(ext), need
        items_p = items.ctypes.data_as(ctypes.POINTER(lib_mod.ProveItem))
        h_proofs, h_commits = np.zeros((n, plen), dtype=np.uint8), np.zeros((n, m, 32), dtype=np.uint8)
        h_lens = np.zeros(n, dtype=np.uintp)
        lens_p = h_lens.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t))
        err = ctypes.create_string_buffer(256)
        mixed_host = packed.MixedInput(h_proofs, np.full(n, plen, dtype=np.uintp), ms, h_commits, minv, minp, seeds if sh["nonces"] else None,
                                       bench.LABEL)
        # device arm: the same rows resident, outputs in device memory
        dev = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()  # noqa: E731
        inp = packed.DeviceOpenings(dev(values), dev(blind), ms, min_values=dev(minv), min_present=dev(minp),
                                    seed_nonces=dev(seeds) if sh["nonces"] else None, rng_bytes=dev(ext), label=bench.LABEL)
        d_proofs = torch.zeros((n, plen), dtype=torch.uint8, device="cuda")
        d_commits = torch.zeros((n, 32 * m), dtype=torch.uint8, device="cuda")
        d_status = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def host_prove():
            rc = lib.bpp_prove_openings(eng.ctx, params.handle, items_p, n, h_commits.ctypes.data, 32 * m, h_proofs.ctypes.data, plen, lens_p,
                                        None, err, 256)
            assert rc == 0, err.value

        def device_prove():
            res = packed.prove_openings_device(params, inp, commitments_out=d_commits, proofs_out=d_proofs, status_out=d_status)
            assert res.rc == 0, res.message
            return res

        def upload(fn, struct):
            h = ctypes.c_uint64()
            rc = fn(eng.ctx, params.handle, ctypes.byref(struct), ctypes.byref(h), err, 256)
            assert rc == 0, err.value
            lib.bpp_batch_destroy(eng.ctx, h)

        first = device_prove()
        mixed_dev = first.as_mixed_input()
        host_prove()
        assert np.array_equal(d_proofs.cpu().numpy(), h_proofs) and np.array_equal(d_commits.cpu().numpy().reshape(n, m, 32), h_commits)
        arms = {"host": host_prove, "device": device_prove,
                "host+upload": lambda: (host_prove(), upload(lib.bpp_batch_upload_mixed, mixed_host.struct)),
                "device+upload": lambda: (device_prove(), upload(lib.bpp_batch_upload_mixed_device, mixed_dev.struct))}
        for fn in arms.values():  # warm-up: both arms, twice
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
        row = {"shape": name, "m": m, "t": t, "nonces": sh["nonces"], "arms": {}}
        for k, v in per.items():
            med = statistics.median(v)
            row["arms"][k] = {"ms_per_call": med, "ms_low": min(v), "ms_high": max(v), "proofs_per_s": n / med * 1e3}
        run["shapes"].append(row)
    run["stats"] = packed.prove_device_stats(eng)
    runs = json.load(open(args.out)) if os.path.exists(args.out) else []
    runs.append(run)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(runs, open(args.out, "w"), indent=1)
    print(json.dumps({"tool": "bench_prove_device", "shapes": {r["shape"]: {k: round(a["ms_per_call"], 3) for k, a in r["arms"].items()}
                                                              for r in run["shapes"]}}))
    eng.close()


if __name__ == "__main__":
    main()
