"""GPU tests of the self-check's replay of mask recovery ("prove_check" = 1 with "prove_check_recovery" = 1): for every proof made
with a seed nonce the checking batch runs under RecoverAndVerify and the recovered masks are compared, on the device, with the
witness's blinding factors.  A checked call returns the bytes of an unchecked one; a disagreement (the test knob
"prove_check_tamper_nonce": one byte XORed into the check's own copy of an item's nonce, never the device's work or the caller's
memory) is located, the proof made again once, and a second disagreement fails that item alone with BPP_ERR_SELF_CHECK (-5) and a
message that names mask recovery.  Calls without a nonce, and calls with "prove_check" off, are left exactly as they were."""
import ctypes
import importlib
import random
import threading

import pytest

from oracle.pyref import curve as C
from oracle.pyref import merlin as M
from oracle.pyref import protocol as O
from tests.helpers import LABEL, Prng, sb

pytestmark = pytest.mark.gpu

STRIDE = 1 + 32 * (6 + 5 + 2 * 12)  # the longest proof any parameters make
SELF_CHECK = -5
STATS = ("calls", "proofs", "batch_failures", "remade", "failed")
RSTATS = ("replayed", "mismatched")
N, M_MAX = 64, 4


def _items(bpp, params, n, t, ms, seed, state=None, promises=True):
    """(transcript, statement, witness, rng bytes) per entry of ms, with the raw values; a canonical seed nonce on every m = 1
    item; every fourth item on `state` (if given)"""
    rng = Prng(seed)
    out = []
    for i, m in enumerate(ms):
        rounds = (n * m).bit_length() - 1
        vals = [rng.next_u64() % (1 << (n - 1)) for _ in range(m)]
        blinds = [[sb(O.random_not_zero(rng)) for _ in range(t)] for _ in range(m)]
        mins = [(v // 3 if promises else None) for v in vals]
        ext = rng.fill_bytes(32 * (rounds + 3))
        nonce = sb(O.random_not_zero(rng)) if m == 1 else None
        comms = params.commit_many(vals, blinds)
        st = bpp.RangeStatement.init(params, comms, mins, nonce)
        w = bpp.RangeWitness.init([bpp.CommitmentOpening.new(vals[j], blinds[j]) for j in range(m)])
        on_state = state is not None and i % 4 == 1
        tr = bpp.Transcript.from_state(state) if on_state else bpp.Transcript.new(LABEL)
        out.append(dict(tr=tr, st=st, w=w, ext=ext, vals=vals, blinds=blinds, mins=mins, comms=comms, m=m, on_state=on_state,
                        nonce=nonce))
    return out


def _marshal(bpp, items):
    return bpp.RangeProof._prove_marshal([x["tr"] for x in items], [x["st"] for x in items], [x["w"] for x in items],
                                         [x["ext"] for x in items])


def _uniform(engine, marshalled, sentinel=0xA5):
    """bpp_prove_batch into a buffer filled with `sentinel` -> (rc, proofs, message, the whole buffer)"""
    params, items, n, _keep = marshalled
    out = (ctypes.c_uint8 * (STRIDE * n))(*([sentinel] * (STRIDE * n)))
    plen = ctypes.c_size_t()
    err = ctypes.create_string_buffer(256)
    rc = engine.lib.bpp_prove_batch(engine.ctx, params.handle, items, n, out, STRIDE, ctypes.byref(plen), err, 256)
    raw = bytes(out)
    return rc, [raw[i * STRIDE:i * STRIDE + plen.value] for i in range(n)], err.value.decode(), raw


def _mixed(engine, marshalled):
    """bpp_prove_batch_mixed -> (rc, proofs, item statuses, proof lengths)"""
    params, items, n, _keep = marshalled
    out = (ctypes.c_uint8 * (STRIDE * n))(*([0xA5] * (STRIDE * n)))
    lens = (ctypes.c_size_t * n)()
    status = (ctypes.c_int * n)()
    err = ctypes.create_string_buffer(256)
    rc = engine.lib.bpp_prove_batch_mixed(engine.ctx, params.handle, items, n, out, STRIDE, lens, status, err, 256)
    raw = bytes(out)
    return rc, [raw[i * STRIDE:i * STRIDE + lens[i]] for i in range(n)], list(status), list(lens)


def _delta(before, after, keys=STATS):
    return {k: after[k] - before[k] for k in keys}


def _rdelta(before, after):
    return _delta(before, after, RSTATS)


def _no_secrets_left(engine):
    examined, nonzero = ctypes.c_uint64(), ctypes.c_uint64()
    assert engine.lib.bpp_prove_secret_bytes(engine.ctx, ctypes.byref(examined), ctypes.byref(nonzero)) == 0
    assert examined.value > 0 and nonzero.value == 0


def _state():
    t0 = M.Transcript(b"outer protocol")
    t0.append_message(b"ctx", b"self-checked outputs with nonces")
    return t0.strobe.to_bytes()


def _tamper_nonce(opt, k, times):
    opt("prove_check_tamper", k + 1)
    opt("prove_check_tamper_nonce", 1)
    opt("prove_check_tamper_byte", 0)
    opt("prove_check_tamper_xor", 1)
    opt("prove_check_tamper_times", times)


UCOUNT = 64
_CACHE = {}


def _params(bpp, engine, n, t):
    key = ("p", n, t)
    if key not in _CACHE:
        _CACHE[key] = bpp.RangeParameters.init(n, M_MAX, bpp.create_pedersen_gens_with_extension_degree(t), engine=engine)
    return _CACHE[key]


def _nonce_case(bpp, engine, t):
    """64 x (n = 64, m = 1), a seed nonce on each, every fourth on a 203-byte transcript state"""
    key = ("u", t)
    if key not in _CACHE:
        params = _params(bpp, engine, N, t)
        items = _items(bpp, params, N, t, [1] * UCOUNT, b"recovery-uniform-%d" % t, _state())
        _CACHE[key] = (params, items, _marshal(bpp, items))
    return _CACHE[key]


def _sample(items):
    """the label items of a stride-9 sample (the oracle helpers below take a label): 0, 18, 27, 36, 54, 63 of 64 -- 9 and 45 sit on
    the state (i % 4 == 1)"""
    return [i for i in range(0, len(items), 9) if not items[i]["on_state"]]


def _oracle_statement(n, t, it):
    op = O.RangeParameters(n, M_MAX, O.PedersenGens(t))
    ost = O.RangeStatement(op, [C.decompress(c) for c in it["comms"]], it["mins"],
                           None if it["nonce"] is None else int.from_bytes(it["nonce"], "little"))
    ow = O.RangeWitness([O.CommitmentOpening(it["vals"][j], [int.from_bytes(x, "little") for x in it["blinds"][j]])
                         for j in range(it["m"])])
    return ost, ow


MS = [4, 1, 2, 1, 4, 1, 2, 1]
WRONG_OPENING, TAMPERED = 5, 3  # (both m = 1 items with a nonce)
XT = 2


def _mixed_case(bpp, engine):
    if "x" not in _CACHE:
        params = _params(bpp, engine, N, XT)
        items = _items(bpp, params, N, XT, MS, b"recovery-mixed", _state())
        bad = items[WRONG_OPENING]
        bad["w"] = bpp.RangeWitness.init([bpp.CommitmentOpening.new(bad["vals"][0] ^ 1, bad["blinds"][0])])
        bad["st"] = bpp.RangeStatement.init(params, bad["comms"], [None], bad["nonce"])
        _CACHE["x"] = (params, items, _marshal(bpp, items))
    return _CACHE["x"]


@pytest.mark.parametrize("t", [1, 3])
def test_bytes_unchanged_and_every_nonce_replayed(bpp, engine, opt, t):
    params, items, mar = _nonce_case(bpp, engine, t)
    rc0, off, msg, _ = _uniform(engine, mar)
    assert rc0 == 0, msg
    opt("prove_check", 1)
    rc1, on, msg, _ = _uniform(engine, mar)
    assert rc1 == 0, msg
    opt("prove_check_recovery", 1)
    s0, r0 = engine.prove_check_stats(), engine.prove_check_recovery_stats()
    rc2, both, msg, _ = _uniform(engine, mar)
    assert rc2 == 0, msg
    assert off == on == both
    assert _delta(s0, engine.prove_check_stats()) == dict(calls=1, proofs=UCOUNT, batch_failures=0, remade=0, failed=0)
    assert _rdelta(r0, engine.prove_check_recovery_stats()) == dict(replayed=UCOUNT, mismatched=0)
    _no_secrets_left(engine)
    sample = _sample(items)
    assert len(sample) >= 4
    for i in sample:
        ost, ow = _oracle_statement(N, t, items[i])
        want = O.prove_with_rng(M.Transcript(LABEL), ost, ow, M.ByteStreamRng(items[i]["ext"])).to_bytes()
        assert both[i] == want, "proof %d differs from the oracle's" % i


@pytest.mark.parametrize("t", [1, 3])
def test_oracle_recovers_the_witness_blinding_factors(bpp, engine, t):
    """the property the replay is about, held to the oracle's verifier (no option of the check is involved)"""
    params, items, mar = _nonce_case(bpp, engine, t)
    rc, proofs, msg, _ = _uniform(engine, mar)
    assert rc == 0, msg
    sample = _sample(items)
    assert len(sample) >= 4
    for i in sample:
        ost, _ow = _oracle_statement(N, t, items[i])
        masks = O.verify([M.Transcript(LABEL)], [ost], [O.RangeProof.from_bytes(proofs[i])], 2)  # RecoverOnly
        assert masks[0] is not None and [sb(x) for x in masks[0]] == items[i]["blinds"][0], i


@pytest.mark.parametrize("times", [1, 2])
def test_disagreement_is_located_and_remade(bpp, engine, opt, times):
    params, items, mar = _nonce_case(bpp, engine, 3)
    _, clean, _, _ = _uniform(engine, mar)
    k = 5
    opt("prove_check", 1)
    opt("prove_check_recovery", 1)
    _tamper_nonce(opt, k, times)
    s0, r0 = engine.prove_check_stats(), engine.prove_check_recovery_stats()
    rc, got, msg, raw = _uniform(engine, mar)
    d, r = _delta(s0, engine.prove_check_stats()), _rdelta(r0, engine.prove_check_recovery_stats())
    assert r == dict(replayed=UCOUNT, mismatched=1)
    if times == 1:
        assert rc == 0, msg
        assert got == clean
        assert d == dict(calls=1, proofs=UCOUNT, batch_failures=1, remade=1, failed=0)
    else:
        assert rc == SELF_CHECK
        assert "proof %d " % k in msg and "mask recovery" in msg, msg
        assert raw == bytes([0xA5]) * len(raw), "a failed call wrote proof bytes"
        assert d == dict(calls=1, proofs=UCOUNT, batch_failures=1, remade=1, failed=1)
    _no_secrets_left(engine)
    # the knobs acted on that call only
    s0, r0 = engine.prove_check_stats(), engine.prove_check_recovery_stats()
    rc, again, msg, _ = _uniform(engine, mar)
    assert rc == 0 and again == clean, msg
    assert _delta(s0, engine.prove_check_stats()) == dict(calls=1, proofs=UCOUNT, batch_failures=0, remade=0, failed=0)
    assert _rdelta(r0, engine.prove_check_recovery_stats()) == dict(replayed=UCOUNT, mismatched=0)
    _no_secrets_left(engine)


def test_mixed_call(bpp, engine, opt):
    params, items, mar = _mixed_case(bpp, engine)
    rc0, off, st0, lens0 = _mixed(engine, mar)
    assert st0[WRONG_OPENING] == 2 and rc0 == 2 and sum(1 for s in st0 if s == 0) == len(MS) - 1
    valid_m1 = sum(1 for i, m in enumerate(MS) if m == 1 and i != WRONG_OPENING)
    opt("prove_check", 1)
    opt("prove_check_recovery", 1)
    s0, r0 = engine.prove_check_stats(), engine.prove_check_recovery_stats()
    rc1, on, st1, lens1 = _mixed(engine, mar)
    assert (rc1, st1, lens1) == (rc0, st0, lens0)
    assert on == off
    assert _delta(s0, engine.prove_check_stats()) == dict(calls=1, proofs=len(MS) - 1, batch_failures=0, remade=0, failed=0)
    assert _rdelta(r0, engine.prove_check_recovery_stats()) == dict(replayed=valid_m1, mismatched=0)
    _no_secrets_left(engine)
    k = TAMPERED
    _tamper_nonce(opt, k, 2)
    s0, r0 = engine.prove_check_stats(), engine.prove_check_recovery_stats()
    rc, got, st, lens = _mixed(engine, mar)
    assert lens == lens0
    assert st[k] == SELF_CHECK and [s for i, s in enumerate(st) if i != k] == [s for i, s in enumerate(st0) if i != k]
    assert rc == st[min(k, WRONG_OPENING)]
    assert got[k] == bytes(lens[k]), "the failed item's slot is not zeroed"
    assert [g for i, g in enumerate(got) if i != k] == [g for i, g in enumerate(off) if i != k]
    assert _delta(s0, engine.prove_check_stats()) == dict(calls=1, proofs=len(MS) - 1, batch_failures=1, remade=1, failed=1)
    assert _rdelta(r0, engine.prove_check_recovery_stats()) == dict(replayed=valid_m1, mismatched=1)
    err = ctypes.create_string_buffer(256)
    code = engine.lib.bpp_prove_item_message(engine.ctx, params.handle, ctypes.byref(mar[1][k]), STRIDE, st[k], err, 256)
    assert code == SELF_CHECK and b"self-check" in err.value and b"mask recovery" in err.value, err.value
    _no_secrets_left(engine)


def test_no_nonce_no_difference(bpp, engine, opt):
    """the uniform shape of tests/test_gpu_prove_check.py (m = 4, t = 3): no item can carry a nonce"""
    params = _params(bpp, engine, N, 3)
    items = _items(bpp, params, N, 3, [4] * UCOUNT, b"recovery-none", _state())
    assert all(x["nonce"] is None for x in items)
    mar = _marshal(bpp, items)
    rc0, off, msg, _ = _uniform(engine, mar)
    assert rc0 == 0, msg
    opt("prove_check", 1)
    s0 = engine.prove_check_stats()
    rc1, on, msg, _ = _uniform(engine, mar)
    alone = _delta(s0, engine.prove_check_stats())
    assert rc1 == 0, msg
    opt("prove_check_recovery", 1)
    s0, r0 = engine.prove_check_stats(), engine.prove_check_recovery_stats()
    rc2, both, msg, _ = _uniform(engine, mar)
    assert rc2 == 0, msg
    assert off == on == both
    assert _delta(s0, engine.prove_check_stats()) == alone == dict(calls=1, proofs=UCOUNT, batch_failures=0, remade=0, failed=0)
    assert _rdelta(r0, engine.prove_check_recovery_stats()) == dict(replayed=0, mismatched=0)
    _no_secrets_left(engine)


def test_pool_replays_every_nonce_it_serves(bpp, engine, opt):
    params = _params(bpp, engine, N, XT)
    ms = [1, 2, 1, 4, 1, 2, 1, 4, 1, 1]
    items = _items(bpp, params, N, XT, ms, b"recovery-pool", _state())
    rc, clean, st0, _ = _mixed(engine, _marshal(bpp, items))  # unchecked
    assert rc == 0 and not any(st0)
    opt("prove_check", 1)  # before the pool is made: its lanes copy the options
    opt("prove_check_recovery", 1)
    pool = importlib.import_module("bulletproofs-plus_amd.packed").ProvePool(params, lanes=2, max_wait_us=300)
    s0, r0 = pool.check_stats(), pool.check_recovery_stats()
    errors, served, nonces = [], [0] * 8, [0] * 8
    barrier = threading.Barrier(8)

    def worker(w):
        r = random.Random(w)
        barrier.wait()
        for _ in range(6):
            pick = [r.randrange(len(items)) for _ in range(r.choice((1, 1, 2, 3)))]
            sel = [items[i] for i in pick]
            try:
                got = pool.prove([x["tr"] for x in sel], [x["st"] for x in sel], [x["w"] for x in sel], [x["ext"] for x in sel])
            except Exception as e:  # noqa: BLE001 (recorded, the test fails below)
                errors.append((w, pick, repr(e)))
                continue
            served[w] += len(pick)
            nonces[w] += sum(1 for x in sel if x["nonce"] is not None)
            if got != [clean[i] for i in pick]:
                errors.append((w, pick, "bytes differ"))

    ts = [threading.Thread(target=worker, args=(w,)) for w in range(8)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    d, r = _delta(s0, pool.check_stats()), _rdelta(r0, pool.check_recovery_stats())
    pool.close()
    assert not errors, errors[:3]
    assert d["proofs"] == sum(served) and d["batch_failures"] == d["remade"] == d["failed"] == 0, d
    assert sum(nonces) > 0 and r == dict(replayed=sum(nonces), mismatched=0), (r, sum(nonces))


def test_highest_extension_degree(bpp, engine, opt):
    n, t = 8, 6
    params = _params(bpp, engine, n, t)
    items = _items(bpp, params, n, t, [1] * 8, b"recovery-t6")
    mar = _marshal(bpp, items)
    rc, clean, msg, _ = _uniform(engine, mar)
    assert rc == 0, msg
    opt("prove_check", 1)
    opt("prove_check_recovery", 1)
    _tamper_nonce(opt, 2, 1)
    s0, r0 = engine.prove_check_stats(), engine.prove_check_recovery_stats()
    rc, got, msg, _ = _uniform(engine, mar)
    assert rc == 0, msg
    assert got == clean
    assert _delta(s0, engine.prove_check_stats()) == dict(calls=1, proofs=8, batch_failures=1, remade=1, failed=0)
    assert _rdelta(r0, engine.prove_check_recovery_stats()) == dict(replayed=8, mismatched=1)
    _no_secrets_left(engine)


def test_off_means_off(bpp, engine, opt):
    params, items, mar = _nonce_case(bpp, engine, 3)
    rc0, off, msg, _ = _uniform(engine, mar)
    assert rc0 == 0, msg
    opt("prove_check", 0)
    opt("prove_check_recovery", 1)
    s0, r0 = engine.prove_check_stats(), engine.prove_check_recovery_stats()
    rc1, got, msg, _ = _uniform(engine, mar)
    assert rc1 == 0, msg
    assert got == off
    assert _delta(s0, engine.prove_check_stats()) == dict.fromkeys(STATS, 0)
    assert _rdelta(r0, engine.prove_check_recovery_stats()) == dict.fromkeys(RSTATS, 0)
