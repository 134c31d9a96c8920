#!/usr/bin/env python3
"""Many threads making one-proof prove calls of mixed aggregation factors (m drawn from {1, 2, 4}, 64-bit, extension degree 1
and 3): S threads, K calls each, in two setups --
  solo:   one context per thread, one bpp_prove_batch per call;
  pooled: one bpp_prove_pool (the calls that wait are proved as one bpp_prove_batch_mixed).
One JSON line per (setup, S, t): proofs/s and p50 / p99 call latency.

  --mixed-ab   instead: one mixed call of 512 x m1 + 256 x m2 + 256 x m4 against the same proofs as one bpp_prove_batch per
               class, one after the other (median of --reps calls each, t = 1 and 3)
  --check      every context (the solo ones, the pool's lanes) verifies each proof before returning it ("prove_check" = 1); the
               pooled lines add the lanes' check counters
  --check-recovery   with --check: mask recovery replayed for the proofs that carry a seed nonce ("prove_check_recovery" = 1)
  --nonces     the rate runs' one-proof calls are all m = 1 with a seed nonce each (otherwise only every third is)
  --openings   the rate runs' calls prove from the openings alone: one bpp_prove_openings (solo) / bpp_prove_pool_openings (pooled)
               per call, the commitments made by the engine
  --openings-two-call   the same output the way it took two calls: bpp_pedersen_commit for the item's openings, then the existing
               prove call, timed together (pooled: the commit call goes to the context the pool was made from, the one context a
               pool's callers share)
  --soak SEC   instead: SEC seconds of 16 threads through the pool, about 5 % of the calls invalid (one item short of external
               randomness); every proof is compared with the bytes of a one-item bpp_prove_batch of the same item on the same GPU
               (not with the CPU oracle: the tests pin both paths to it), every error with that of a call of its own
"""
import argparse
import ctypes
import importlib
import json
import os
import random
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LABEL = b"bench_prove_pool"


def corpus(bpp, params, n, t, count, seed, nonces=False):
    """count (transcript, statement, witness, rng) of m = 1, 2, 4 in turn, seed nonces on the m = 1 ones (nonces: all m = 1)"""
    r = random.Random(seed)
    out = []
    for i in range(count):
        m = 1 if nonces else (1, 2, 4)[i % 3]
        rounds = (n * m).bit_length() - 1
        vals = [r.getrandbits(n - 1) for _ in range(m)]
        blinds = [[(r.getrandbits(250) + 1).to_bytes(32, "little") for _ in range(t)] for _ in range(m)]
        comms = params.commit_many(vals, blinds)
        snonce = (r.getrandbits(250) + 1).to_bytes(32, "little") if m == 1 else None
        st = bpp.RangeStatement.init(params, comms, [v // 3 for v in vals], snonce)
        w = bpp.RangeWitness.init([bpp.CommitmentOpening.new(vals[j], blinds[j]) for j in range(m)])
        out.append((bpp.Transcript.new(LABEL), st, w, bytes(r.getrandbits(8) for _ in range(32 * (rounds + 3)))))
    return out


def marshal(bpp, items):
    return bpp.RangeProof._prove_marshal([x[0] for x in items], [x[1] for x in items], [x[2] for x in items], [x[3] for x in items])


STRIDE = 1 + 32 * (6 + 5 + 2 * 12)


def solo_call(eng, params, mar):
    _p, arr, n, _k = mar
    out = (ctypes.c_uint8 * (STRIDE * n))()
    plen = ctypes.c_size_t()
    err = ctypes.create_string_buffer(256)
    rc = eng.lib.bpp_prove_batch(eng.ctx, params.handle, arr, n, out, STRIDE, ctypes.byref(plen), err, 256)
    assert rc == 0, err.value
    raw = bytes(out)
    return [raw[i * STRIDE:i * STRIDE + plen.value] for i in range(n)]


def openings_call(eng, params, mar):
    """one bpp_prove_openings over items marshalled without commitments -> proof bytes"""
    _p, arr, n, _k = mar
    out = (ctypes.c_uint8 * (STRIDE * n))()
    comms = (ctypes.c_uint8 * (128 * n))()
    lens = (ctypes.c_size_t * n)()
    err = ctypes.create_string_buffer(256)
    rc = eng.lib.bpp_prove_openings(eng.ctx, params.handle, arr, n, comms, 128, out, STRIDE, lens, None, err, 256)
    assert rc == 0, err.value
    raw = bytes(out)
    return [raw[i * STRIDE:i * STRIDE + lens[i]] for i in range(n)]


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))]


def run_threads(S, fn):
    lat = [[] for _ in range(S)]
    bar = threading.Barrier(S + 1)

    def worker(k):
        bar.wait()
        fn(k, lat[k])
    th = [threading.Thread(target=worker, args=(k,)) for k in range(S)]
    for x in th:
        x.start()
    bar.wait()
    t0 = time.perf_counter()
    for x in th:
        x.join()
    return time.perf_counter() - t0, [v for row in lat for v in row]


def bench_rates(bpp, packed, args):
    for t in args.t:
        eng0 = bpp.Engine(0)
        if args.check:
            eng0.set_option("prove_check", 1)  # (before the pools are made: their lanes copy it)
        if args.check_recovery:
            eng0.set_option("prove_check_recovery", 1)
        p0 = bpp.RangeParameters.init(64, 4, bpp.create_pedersen_gens_with_extension_degree(t), engine=eng0)
        raw = corpus(bpp, p0, 64, t, 48, t, args.nonces)
        items = [marshal(bpp, [x]) for x in raw]
        # the same items without commitments, and their openings for the two-call form's bpp_pedersen_commit
        bare = [bpp.RangeProof._openings_marshal([x[0]], [x[2]], [x[1].minimum_value_promises], [x[1].seed_nonce], [x[3]], p0) for x in raw]
        opened = [([o.v for o in x[2].openings], [o.r for o in x[2].openings]) for x in raw]
        solo_call(eng0, p0, items[0])  # fixed-base table, arena
        for S in args.threads:
            for setup in ("solo", "pooled"):
                if setup == "solo":
                    engs = [bpp.Engine(0) for _ in range(S)]
                    for e in engs if args.check else ():
                        e.set_option("prove_check", 1)
                    for e in engs if args.check_recovery else ():
                        e.set_option("prove_check_recovery", 1)
                    ps = [p0.share(e) for e in engs]
                    for k in range(S):
                        solo_call(engs[k], ps[k], items[k % len(items)])

                    def fn(k, lat):
                        for c in range(args.calls):
                            i = (k * 7 + c) % len(items)
                            a = time.perf_counter()
                            if args.openings:
                                openings_call(engs[k], ps[k], bare[i])
                            else:
                                if args.openings_two_call:
                                    ps[k].commit_many(*opened[i])
                                solo_call(engs[k], ps[k], items[i])
                            lat.append(time.perf_counter() - a)
                else:
                    pool = packed.ProvePool(p0, lanes=args.lanes, max_wait_us=args.max_wait_us)
                    for k in range(2 * args.lanes):
                        pool.prove_marshalled(items[k])

                    def fn(k, lat):
                        for c in range(args.calls):
                            i = (k * 7 + c) % len(items)
                            a = time.perf_counter()
                            if args.openings:
                                pool.prove_openings_marshalled(bare[i])
                            else:
                                if args.openings_two_call:
                                    p0.commit_many(*opened[i])
                                pool.prove_marshalled(items[i])
                            lat.append(time.perf_counter() - a)
                el, lat = run_threads(S, fn)
                rec = {"metric": "one-proof prove calls, " + ("m = 1 with seed nonces" if args.nonces else "m in {1,2,4}"), "setup": setup, "threads": S, "calls_per_thread": args.calls,
                       "bit_length": 64, "extension_degree": t, "proofs_per_s": S * args.calls / el,
                       "p50_ms": 1e3 * pct(lat, 0.5), "p99_ms": 1e3 * pct(lat, 0.99), "prove_check": 1 if args.check else 0,
                       "prove_check_recovery": 1 if args.check_recovery else 0,
                       "form": "openings" if args.openings else ("openings-two-call" if args.openings_two_call else "commitments brought")}
                if setup == "solo":
                    for p in ps:
                        p.close()
                    for e in engs:
                        e.close()
                else:
                    rec.update(pool.stats(), lanes=args.lanes, max_wait_us=args.max_wait_us)
                    if args.check:
                        rec["check"] = pool.check_stats()
                    if args.check_recovery:
                        rec["check_recovery"] = pool.check_recovery_stats()
                    pool.close()
                print(json.dumps(rec), flush=True)
        p0.close()
        eng0.close()


def bench_mixed_ab(bpp, args):
    for t in args.t:
        eng = bpp.Engine(0)
        p = bpp.RangeParameters.init(64, 4, bpp.create_pedersen_gens_with_extension_degree(t), engine=eng)
        base = corpus(bpp, p, 64, t, 48, 100 + t)
        by_m = {m: [x for x in base if len(x[1].commitments_compressed) == m] for m in (1, 2, 4)}
        want = {1: 512, 2: 256, 4: 256}
        items = [by_m[m][k % len(by_m[m])] for m in (1, 2, 4) for k in range(want[m])]
        random.Random(t).shuffle(items)
        mixed = marshal(bpp, items)
        classes = [marshal(bpp, [x for x in items if len(x[1].commitments_compressed) == m]) for m in (1, 2, 4)]
        _p, arr, n, _k = mixed
        out = (ctypes.c_uint8 * (STRIDE * n))()
        lens = (ctypes.c_size_t * n)()
        err = ctypes.create_string_buffer(256)

        def one_mixed():
            assert eng.lib.bpp_prove_batch_mixed(eng.ctx, p.handle, arr, n, out, STRIDE, lens, None, err, 256) == 0, err.value

        def per_class():
            for c in classes:
                solo_call(eng, p, c)
        res = {}
        for name, fn in (("mixed", one_mixed), ("per_class", per_class)):
            fn()
        ts = {"mixed": [], "per_class": []}
        for _ in range(args.reps):  # alternating
            for name, fn in (("mixed", one_mixed), ("per_class", per_class)):
                a = time.perf_counter()
                fn()
                ts[name].append(time.perf_counter() - a)
        for name in ts:
            res[name + "_ms"] = 1e3 * pct(ts[name], 0.5)
        print(json.dumps({"metric": "1024 proofs (512 m1, 256 m2, 256 m4): one ragged mixed call vs one uniform call per class in a row",
                          "extension_degree": t, "reps": args.reps, **res, "mixed_proofs_per_s": 1024e3 / res["mixed_ms"],
                          "per_class_proofs_per_s": 1024e3 / res["per_class_ms"]}), flush=True)
        p.close()
        eng.close()


def soak(bpp, packed, args):
    t = 3
    eng = bpp.Engine(0)
    p = bpp.RangeParameters.init(64, 4, bpp.create_pedersen_gens_with_extension_degree(t), engine=eng)
    items = corpus(bpp, p, 64, t, 60, 7)
    ref_eng = bpp.Engine(0)
    ref_p = p.share(ref_eng)
    ref = [solo_call(ref_eng, ref_p, marshal(bpp, [x]))[0] for x in items]
    mar = [marshal(bpp, [x]) for x in items]
    bad_items = [(x[0], x[1], x[2], x[3][:-32]) for x in items[:6]]
    bad_mar = [marshal(bpp, [x]) for x in bad_items]
    bad_ref = []
    for x in bad_mar:
        _p, arr, n, _k = x
        out = (ctypes.c_uint8 * STRIDE)()
        plen = ctypes.c_size_t()
        err = ctypes.create_string_buffer(256)
        rc = ref_eng.lib.bpp_prove_batch(ref_eng.ctx, ref_p.handle, arr, 1, out, STRIDE, ctypes.byref(plen), err, 256)
        assert rc > 0
        bad_ref.append((rc, err.value.decode()))
    pool = packed.ProvePool(p, lanes=args.lanes, max_wait_us=args.max_wait_us)
    stop = time.time() + args.soak
    counts = [[0, 0, 0] for _ in range(16)]  # proofs, byte mismatches, invalid calls (a wrong outcome counts as a mismatch)

    def fn(k, lat):
        r = random.Random(k)
        while time.time() < stop:
            if r.random() < 0.05:
                b = r.randrange(len(bad_mar))
                try:
                    pool.prove_marshalled(bad_mar[b])
                    got = None
                except bpp.ProofError as e:
                    got = (int(e.kind), e.msg)
                counts[k][2] += 1
                counts[k][1] += got != bad_ref[b]
                continue
            idx = [r.randrange(len(items)) for _ in range(r.choice((1, 1, 2, 3)))]
            if len(idx) == 1:
                got = pool.prove_marshalled(mar[idx[0]])
            else:
                got = pool.prove_marshalled(marshal(bpp, [items[i] for i in idx]))
            for g, i in zip(got, idx):
                counts[k][0] += 1
                counts[k][1] += g != ref[i]
    el, _ = run_threads(16, fn)
    st = pool.stats()
    pool.close()
    proofs, bad, invalid = sum(c[0] for c in counts), sum(c[1] for c in counts), sum(c[2] for c in counts)
    print(json.dumps({"metric": "prove pool soak, m in {1,2,4}, t = 3, 16 threads", "seconds": el, "proofs": proofs,
                      "invalid_calls": invalid, "mismatches": bad, "compared_with": "one-item bpp_prove_batch, same GPU", **st}),
          flush=True)
    ref_p.close()
    ref_eng.close()
    p.close()
    eng.close()
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", default="16,32")
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--t", default="1,3")
    ap.add_argument("--lanes", type=int, default=2)
    ap.add_argument("--max-wait-us", type=int, default=0)
    ap.add_argument("--mixed-ab", action="store_true")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--soak", type=float, default=0)
    ap.add_argument("--check", action="store_true", help='"prove_check" = 1 on every context of the rate runs')
    ap.add_argument("--check-recovery", action="store_true", help='"prove_check_recovery" = 1 on every context of the rate runs')
    ap.add_argument("--openings", action="store_true", help="rate runs: one call from the openings alone (bpp_prove_openings)")
    ap.add_argument("--openings-two-call", action="store_true", help="rate runs: bpp_pedersen_commit + the existing prove call, timed together")
    ap.add_argument("--nonces", action="store_true", help="rate runs: every call one m = 1 proof with a seed nonce")
    args = ap.parse_args()
    args.threads = [int(x) for x in args.threads.split(",")]
    args.t = [int(x) for x in args.t.split(",")]
    bpp = importlib.import_module("bulletproofs-plus_amd")
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    if args.soak:
        sys.exit(1 if soak(bpp, packed, args) else 0)
    if args.mixed_ab:
        bench_mixed_ab(bpp, args)
    else:
        bench_rates(bpp, packed, args)


if __name__ == "__main__":
    main()
