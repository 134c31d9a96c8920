"""GPU tests of bpp_prove_pool: 16 threads of one process make one- and few-proof calls of random aggregation factors, a few of
them invalid, through one pool; every caller gets the oracle's bytes or the error a call of its own returns, the calls are
pooled, the limits hold, and no witness byte is left behind."""
import ctypes
import importlib
import random
import threading

import pytest

from oracle import cport
from oracle.pyref import protocol as O
from tests.helpers import LABEL, Prng, sb

pytestmark = pytest.mark.gpu

N, M_MAX, T = 8, 4, 1


def _corpus(bpp, params, count, seed):
    """count valid items of m in {1, 2, 4} with the oracle's bytes, each also as an invalid twin (one rng draw short)"""
    rng = Prng(seed)
    cp = cport.Params(N, M_MAX, T)
    out = []
    for i in range(count):
        m = (1, 2, 4)[i % 3]
        rounds = (N * m).bit_length() - 1
        vals = [rng.next_u64() % (1 << N) for _ in range(m)]
        blinds = [[sb(O.random_not_zero(rng))] for _ in range(m)]
        mins = [v // 2 if j == 0 else None for j, v in enumerate(vals)]
        snonce = sb(O.random_not_zero(rng)) if m == 1 else None
        ext = rng.fill_bytes(32 * (rounds + 3))
        comms = params.commit_many(vals, blinds)
        st = bpp.RangeStatement.init(params, comms, mins, snonce)
        w = bpp.RangeWitness.init([bpp.CommitmentOpening.new(vals[j], blinds[j]) for j in range(m)])
        want, _ = cp.prove(LABEL, vals, blinds, mins, snonce, ext)
        out.append(dict(st=st, w=w, ext=ext, want=want))
    cp.close()
    return out


def _expect(bpp, calls):
    """what a call of its own returns for these items: (proof bytes, None) or (None, (kind, msg))"""
    tr = [bpp.Transcript.new(LABEL)] * len(calls)
    got = bpp.RangeProof.prove_batch_mixed(tr, [c["st"] for c in calls], [c["w"] for c in calls], [c["ext"] for c in calls])
    for g in got:
        if isinstance(g, bpp.ProofError):
            return None, (g.kind, g.msg)
    return [g.to_bytes() for g in got], None


def _run(bpp, pool, corpus, threads, calls_per_thread, seed, bad_rate):
    errors = []
    barrier = threading.Barrier(threads)

    def worker(k):
        r = random.Random(seed * 1000 + k)
        barrier.wait()
        for _ in range(calls_per_thread):
            picks = [dict(corpus[r.randrange(len(corpus))]) for _ in range(r.choice((1, 1, 1, 2, 3)))]
            bad = r.random() < bad_rate
            if bad:
                picks[-1]["ext"] = picks[-1]["ext"][:-32]
            tr = [bpp.Transcript.new(LABEL)] * len(picks)
            try:
                got = pool.prove(tr, [p["st"] for p in picks], [p["w"] for p in picks], [p["ext"] for p in picks])
                res = ("ok", got)
            except bpp.ProofError as e:
                res = ("err", (e.kind, e.msg))
            if bad:
                want = ("err", _expect(bpp, picks)[1])
            else:
                want = ("ok", [p["want"] for p in picks])
            if res != want:
                errors.append((k, res, want))

    ts = [threading.Thread(target=worker, args=(k,)) for k in range(threads)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    return errors


def test_prove_pool_many_threads(bpp, engine):
    params = bpp.RangeParameters.init(N, M_MAX, bpp.create_pedersen_gens_with_extension_degree(T), engine=engine)
    corpus = _corpus(bpp, params, 24, b"pool")
    pool = importlib.import_module("bulletproofs-plus_amd.packed").ProvePool(params, lanes=2, max_wait_us=300)
    errors = _run(bpp, pool, corpus, 16, 12, 1, 0.05)
    st = pool.stats()
    pool.close()
    assert not errors, errors[:3]
    calls = st["pooled_calls"] + st["solo_calls"]
    assert calls == 16 * 12
    assert st["engine_calls"] < calls and st["largest_calls"] > 1, st
    examined, nonzero = ctypes.c_uint64(), ctypes.c_uint64()
    assert engine.lib.bpp_prove_secret_bytes(engine.ctx, ctypes.byref(examined), ctypes.byref(nonzero)) == 0
    assert examined.value > 0 and nonzero.value == 0


def test_prove_pool_limits(bpp, engine):
    params = bpp.RangeParameters.init(N, M_MAX, bpp.create_pedersen_gens_with_extension_degree(T), engine=engine)
    corpus = _corpus(bpp, params, 9, b"limits")
    pool = importlib.import_module("bulletproofs-plus_amd.packed").ProvePool(params, lanes=2, max_wait_us=300)
    pool.set_limits(max_calls=2, max_proofs=3)
    errors = _run(bpp, pool, corpus, 16, 4, 2, 0.0)
    st = pool.stats()
    pool.close()
    assert not errors, errors[:3]
    assert 1 < st["largest_calls"] <= 2 and st["largest_proofs"] <= 3, st
    assert st["engine_calls"] < 16 * 4
