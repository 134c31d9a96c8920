"""GPU tests of the prover's self-check ("prove_check" = 1): every proof bpp_prove_batch / bpp_prove_batch_mixed / bpp_prove_pool
make is verified on the context before it is returned.  A checked call returns the same bytes, codes and statuses as an unchecked
one; a proof altered in the host copy (the test knobs "prove_check_tamper*": one byte XORed after the device wrote it, never a
device fault) is located and made again, and one altered again fails alone with BPP_ERR_SELF_CHECK (-5), for each of the three
places a rejection can come from: the final MSM, the decompression of a point on the device, the upload's parser."""
import ctypes
import importlib
import random
import threading

import pytest

from oracle import cport
from oracle.pyref import merlin as M
from oracle.pyref import protocol as O
from tests.helpers import LABEL, Prng, sb

pytestmark = pytest.mark.gpu

STRIDE = 1 + 32 * (6 + 5 + 2 * 12)  # the longest proof any parameters make
SELF_CHECK = -5
STATS = ("calls", "proofs", "batch_failures", "remade", "failed")


def _items(bpp, params, n, t, ms, seed, state=None, promises=True):
    """(transcript, statement, witness, rng bytes) per entry of ms, with the raw values; every fourth item on `state` (if given)"""
    rng = Prng(seed)
    out = []
    for i, m in enumerate(ms):
        rounds = (n * m).bit_length() - 1
        vals = [rng.next_u64() % (1 << (n - 1)) for _ in range(m)]
        blinds = [[sb(O.random_not_zero(rng)) for _ in range(t)] for _ in range(m)]
        mins = [(v // 3 if promises else None) for v in vals]
        ext = rng.fill_bytes(32 * (rounds + 3))
        comms = params.commit_many(vals, blinds)
        st = bpp.RangeStatement.init(params, comms, mins, None)
        w = bpp.RangeWitness.init([bpp.CommitmentOpening.new(vals[j], blinds[j]) for j in range(m)])
        on_state = state is not None and i % 4 == 1
        tr = bpp.Transcript.from_state(state) if on_state else bpp.Transcript.new(LABEL)
        out.append(dict(tr=tr, st=st, w=w, ext=ext, vals=vals, blinds=blinds, mins=mins, comms=comms, m=m, on_state=on_state))
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


def _delta(before, after):
    return {k: after[k] - before[k] for k in STATS}


def _no_secrets_left(engine):
    examined, nonzero = ctypes.c_uint64(), ctypes.c_uint64()
    assert engine.lib.bpp_prove_secret_bytes(engine.ctx, ctypes.byref(examined), ctypes.byref(nonzero)) == 0
    assert examined.value > 0 and nonzero.value == 0


def _state():
    t0 = M.Transcript(b"outer protocol")
    t0.append_message(b"ctx", b"self-checked outputs")
    return t0.strobe.to_bytes()


# uniform: configs[4]'s shape (n = 64, m = 4, t = 3), 64 items with promises, every fourth on a 203-byte transcript state
UN, UM, UT, UCOUNT = 64, 4, 3, 64
# mixed: m in {1, 2, 4, 8}, t = 2; two invalid items among them
XN, XM, XT = 8, 8, 2
XMS = [4, 1, 8, 2, 1, 4, 2, 8, 1, 2, 4, 1]
WRONG_OPENING, SEED_WITH_M2 = 2, 6  # (an m = 8 item whose witness does not open its commitments; an m = 2 item with a seed nonce)
_CACHE = {}


def _uniform_case(bpp, engine):
    if "u" not in _CACHE:
        params = bpp.RangeParameters.init(UN, UM, bpp.create_pedersen_gens_with_extension_degree(UT), engine=engine)
        items = _items(bpp, params, UN, UT, [UM] * UCOUNT, b"check-uniform", _state())
        _CACHE["u"] = (params, items, _marshal(bpp, items))
    return _CACHE["u"]


def _mixed_case(bpp, engine):
    if "x" not in _CACHE:
        params = bpp.RangeParameters.init(XN, XM, bpp.create_pedersen_gens_with_extension_degree(XT), engine=engine)
        items = _items(bpp, params, XN, XT, XMS, b"check-mixed", _state())
        bad = items[WRONG_OPENING]
        bad["w"] = bpp.RangeWitness.init([bpp.CommitmentOpening.new(bad["vals"][j] ^ (1 if j == 0 else 0), bad["blinds"][j])
                                          for j in range(bad["m"])])
        bad["st"] = bpp.RangeStatement.init(params, bad["comms"], [None] * bad["m"], None)
        mar = _marshal(bpp, items)
        seed = (ctypes.c_uint8 * 32)(*sb(12345))
        mar[3].append(seed)
        mar[1][SEED_WITH_M2].seed_nonce32 = ctypes.cast(seed, ctypes.c_void_p)  # (RangeStatement.init refuses it; the engine must too)
        _CACHE["x"] = (params, items, mar)
    return _CACHE["x"]


def test_uniform_checked_bytes_equal_unchecked(bpp, engine, opt):
    params, items, mar = _uniform_case(bpp, engine)
    rc0, off, _, _ = _uniform(engine, mar)
    assert rc0 == 0
    opt("prove_check", 1)
    s0 = engine.prove_check_stats()
    rc1, on, msg, _ = _uniform(engine, mar)
    assert rc1 == 0, msg
    assert on == off
    assert _delta(s0, engine.prove_check_stats()) == dict(calls=1, proofs=UCOUNT, batch_failures=0, remade=0, failed=0)
    # a sample of the label items through the CPU oracle's verifier, as one batch
    cp = cport.Params(UN, UM, UT)
    sample = [i for i in range(0, UCOUNT, 9) if not items[i]["on_state"]]
    rc, _, _ = cp.verify([dict(proof=on[i], commitments=items[i]["comms"], min_values=items[i]["mins"], seed_nonce=None, label=LABEL)
                          for i in sample])
    cp.close()
    assert rc == 0 and len(sample) >= 4


def test_mixed_checked_equals_unchecked_and_counts_valid_items(bpp, engine, opt):
    params, items, mar = _mixed_case(bpp, engine)
    rc0, off, st0, lens0 = _mixed(engine, mar)
    assert st0[WRONG_OPENING] == 2 and st0[SEED_WITH_M2] == 2 and rc0 == st0[min(WRONG_OPENING, SEED_WITH_M2)]
    assert sum(1 for s in st0 if s == 0) == len(XMS) - 2
    opt("prove_check", 1)
    s0 = engine.prove_check_stats()
    rc1, on, st1, lens1 = _mixed(engine, mar)
    assert (rc1, st1, lens1) == (rc0, st0, lens0)
    assert on == off
    assert _delta(s0, engine.prove_check_stats()) == dict(calls=1, proofs=len(XMS) - 2, batch_failures=0, remade=0, failed=0)


def test_ct2_checked_bytes_equal(bpp, engine, opt):
    params, items, mar = _uniform_case(bpp, engine)
    _, want, _, _ = _uniform(engine, mar)
    opt("ct", 2)
    rc0, off, _, _ = _uniform(engine, mar)
    opt("prove_check", 1)
    s0 = engine.prove_check_stats()
    rc1, on, msg, _ = _uniform(engine, mar)
    assert rc0 == rc1 == 0, msg
    assert on == off == want
    assert _delta(s0, engine.prove_check_stats())["proofs"] == UCOUNT


def _sites(t):
    """(byte, mask) per place a rejection comes from: the final MSM (d1[0] stays canonical), the device's decompression (A with
    bit 0 set is no ristretto255 encoding), the upload's parser (d1[0] >= 2^255)"""
    return {"msm": (1, 0x01), "decompress": (1 + 32 * t, 0x01), "upload": (32, 0x80)}


@pytest.mark.parametrize("times", [1, 2])
@pytest.mark.parametrize("site", ["msm", "decompress", "upload"])
def test_uniform_tampered_proof(bpp, engine, opt, site, times):
    params, items, mar = _uniform_case(bpp, engine)
    _, clean, _, _ = _uniform(engine, mar)
    k = 5
    byte, mask = _sites(UT)[site]
    opt("prove_check", 1)
    opt("prove_check_tamper", k + 1)
    opt("prove_check_tamper_byte", byte)
    opt("prove_check_tamper_xor", mask)
    opt("prove_check_tamper_times", times)
    s0 = engine.prove_check_stats()
    rc, got, msg, raw = _uniform(engine, mar)
    d = _delta(s0, engine.prove_check_stats())
    if times == 1:
        assert rc == 0, msg
        assert got == clean
        assert d == dict(calls=1, proofs=UCOUNT, batch_failures=1, remade=1, failed=0)
    else:
        assert rc == SELF_CHECK
        assert "proof %d " % k in msg, msg
        assert raw == bytes([0xA5]) * len(raw), "a failed call wrote proof bytes"
        assert d == dict(calls=1, proofs=UCOUNT, batch_failures=1, remade=1, failed=1)
    _no_secrets_left(engine)
    # the knobs acted on that call only
    rc, again, msg, _ = _uniform(engine, mar)
    assert rc == 0 and again == clean, msg


@pytest.mark.parametrize("times", [1, 2])
@pytest.mark.parametrize("site", ["msm", "decompress", "upload"])
def test_mixed_tampered_proof(bpp, engine, opt, site, times):
    params, items, mar = _mixed_case(bpp, engine)
    rc0, clean, st0, lens0 = _mixed(engine, mar)
    k = 3  # (an m = 2 item, valid; the call sorts it behind the m = 8 and m = 4 items)
    assert st0[k] == 0
    byte, mask = _sites(XT)[site]
    opt("prove_check", 1)
    opt("prove_check_tamper", k + 1)
    opt("prove_check_tamper_byte", byte)
    opt("prove_check_tamper_xor", mask)
    opt("prove_check_tamper_times", times)
    s0 = engine.prove_check_stats()
    rc, got, st, lens = _mixed(engine, mar)
    d = _delta(s0, engine.prove_check_stats())
    assert lens == lens0
    if times == 1:
        assert (rc, st) == (rc0, st0)
        assert got == clean
        assert d == dict(calls=1, proofs=len(XMS) - 2, batch_failures=1, remade=1, failed=0)
    else:
        assert st[k] == SELF_CHECK and [s for i, s in enumerate(st) if i != k] == [s for i, s in enumerate(st0) if i != k]
        assert rc == st[min(k, WRONG_OPENING)]
        assert got[k] == bytes(lens[k]), "the failed item's slot is not zeroed"
        assert [g for i, g in enumerate(got) if i != k] == [g for i, g in enumerate(clean) if i != k]
        assert d == dict(calls=1, proofs=len(XMS) - 2, batch_failures=1, remade=1, failed=1)
        err = ctypes.create_string_buffer(256)
        code = engine.lib.bpp_prove_item_message(engine.ctx, params.handle, ctypes.byref(mar[1][k]), STRIDE, st[k], err, 256)
        assert code == SELF_CHECK and b"self-check" in err.value
    _no_secrets_left(engine)


def test_self_check_failure_through_the_python_api(bpp, engine, opt):
    params, items, mar = _mixed_case(bpp, engine)
    valid = [x for i, x in enumerate(items) if i not in (WRONG_OPENING, SEED_WITH_M2) and x["m"] == 4]
    opt("prove_check", 1)
    for name, value in (("prove_check_tamper", 2), ("prove_check_tamper_times", 2)):
        opt(name, value)
    with pytest.raises(bpp.EngineError) as e:
        bpp.RangeProof.prove_batch([x["tr"] for x in valid], [x["st"] for x in valid], [x["w"] for x in valid], [x["ext"] for x in valid])
    assert e.value.code == SELF_CHECK
    for name, value in (("prove_check_tamper", 2), ("prove_check_tamper_times", 2)):
        opt(name, value)
    got = bpp.RangeProof.prove_batch_mixed([x["tr"] for x in valid], [x["st"] for x in valid], [x["w"] for x in valid],
                                           [x["ext"] for x in valid])
    assert isinstance(got[1], bpp.EngineError) and got[1].code == SELF_CHECK
    assert all(isinstance(g, bpp.RangeProof) for i, g in enumerate(got) if i != 1)


def test_pool_checks_every_proof_it_serves(bpp, engine, opt):
    params, items, mar = _mixed_case(bpp, engine)
    valid = [i for i in range(len(XMS)) if i not in (WRONG_OPENING, SEED_WITH_M2)]
    _, clean, st0, _ = _mixed(engine, mar)  # unchecked
    opt("prove_check", 1)  # before the pool is made: its lanes copy the option
    pool = importlib.import_module("bulletproofs-plus_amd.packed").ProvePool(params, lanes=2, max_wait_us=300)
    s0 = pool.check_stats()
    errors, served = [], [0] * 8
    barrier = threading.Barrier(8)

    def worker(w):
        r = random.Random(w)
        barrier.wait()
        for _ in range(6):
            pick = [valid[r.randrange(len(valid))] for _ in range(r.choice((1, 1, 2, 3)))]
            sel = [items[i] for i in pick]
            try:
                got = pool.prove([x["tr"] for x in sel], [x["st"] for x in sel], [x["w"] for x in sel], [x["ext"] for x in sel])
            except Exception as e:  # noqa: BLE001 (recorded, the test fails below)
                errors.append((w, pick, repr(e)))
                continue
            served[w] += len(pick)
            if got != [clean[i] for i in pick]:
                errors.append((w, pick, "bytes differ"))

    ts = [threading.Thread(target=worker, args=(w,)) for w in range(8)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    d = _delta(s0, pool.check_stats())
    st = pool.stats()
    pool.close()
    assert not errors, errors[:3]
    assert d["proofs"] == sum(served) and d["calls"] >= 1, d
    assert d["batch_failures"] == d["remade"] == d["failed"] == 0, d
    assert st["engine_calls"] < 8 * 6, st


def test_default_context_checks_nothing(bpp):
    eng = bpp.Engine(0)
    try:
        params = bpp.RangeParameters.init(8, 2, bpp.create_pedersen_gens_with_extension_degree(1), engine=eng)
        its = _items(bpp, params, 8, 1, [2, 2, 2], b"check-default")
        got = bpp.RangeProof.prove_batch([x["tr"] for x in its], [x["st"] for x in its], [x["w"] for x in its], [x["ext"] for x in its])
        assert len(got) == 3
        assert eng.prove_check_stats() == dict.fromkeys(STATS, 0)
        params.close()
    finally:
        eng.close()
