"""GPU tests of proving from the openings alone (bpp_prove_openings, bpp_prove_pool_openings): an item without commitments has
them made by the engine where the prover's witness check computes them anyway.  The commitments are the oracle's, the proofs the
oracle prover's and those of bpp_prove_batch_mixed over the same items with the commitments filled in, under "ct" = 0, 1, 2; items
of both kinds share ragged calls and pooled calls; failures stay with their item; the self-check works on the made commitments;
no witness byte is left behind; the existing entry points still refuse an item without commitments."""
import ctypes
import importlib
import random
import threading

import pytest

from oracle import cport
from oracle.pyref import curve as C
from oracle.pyref import merlin as M
from oracle.pyref import protocol as O
from tests.helpers import LABEL, Prng, sb

pytestmark = pytest.mark.gpu

STRIDE = 1 + 32 * (6 + 5 + 2 * 12)  # the longest proof any parameters make
SELF_CHECK, INVALID_ARGUMENT, INVALID_LENGTH = -5, 2, 3
STATS = ("calls", "proofs", "batch_failures", "remade", "failed")
N, M_MAX = 64, 8
L_ORDER = 2 ** 252 + 27742317777372353535851937790883648493
_CACHE = {}


def _params(bpp, engine, t):
    if ("p", t) not in _CACHE:
        _CACHE[("p", t)] = bpp.RangeParameters.init(N, M_MAX, bpp.create_pedersen_gens_with_extension_degree(t), engine=engine)
    return _CACHE[("p", t)]


def _state():
    t0 = M.Transcript(b"outer protocol")
    t0.append_message(b"ctx", b"outputs made from openings")
    return t0


def _item(bpp, t, m, vals, blinds, mins, nonce, ext, state=None):
    """one item as the tests pass it around: the openings, the promises, the transcript; nothing of it is a commitment"""
    w = bpp.RangeWitness.init([bpp.CommitmentOpening.new(vals[j], blinds[j]) for j in range(m)])
    tr = bpp.Transcript.from_state(state.strobe.to_bytes()) if state is not None else bpp.Transcript.new(LABEL)
    return dict(tr=tr, w=w, ext=ext, vals=vals, blinds=blinds, mins=mins, nonce=nonce, m=m, t=t, state=state)


def _items(bpp, t, ms, seed, promises=True, nonces=False, state_every=0):
    rng = Prng(seed)
    out = []
    for i, m in enumerate(ms):
        rounds = (N * m).bit_length() - 1
        vals = [rng.next_u64() % (1 << (N - 1)) for _ in range(m)]
        blinds = [[sb(O.random_not_zero(rng)) for _ in range(t)] for _ in range(m)]
        mins = [(v // 3 if promises and (i + j) % 2 == 0 else None) for j, v in enumerate(vals)]
        nonce = sb(O.random_not_zero(rng)) if nonces and m == 1 else None
        ext = rng.fill_bytes(32 * (rounds + 3))
        state = _state() if state_every and i % state_every == state_every - 1 else None
        out.append(_item(bpp, t, m, vals, blinds, mins, nonce, ext, state))
    return out


def _oracle(it, cp):
    """the oracle's (commitments, proof bytes) for an item: oracle.cport for a label, oracle.pyref for a transcript state"""
    if it["state"] is None:
        proof, comms = cp.prove(LABEL, it["vals"], it["blinds"], it["mins"], it["nonce"], it["ext"])
        return [bytes(c) for c in comms], proof
    comms = [cp.commit(it["vals"][j], it["blinds"][j]) for j in range(it["m"])]
    op = O.RangeParameters(N, M_MAX, O.PedersenGens(it["t"]))
    ost = O.RangeStatement(op, [C.decompress(c) for c in comms], it["mins"],
                           None if it["nonce"] is None else int.from_bytes(it["nonce"], "little"))
    ow = O.RangeWitness([O.CommitmentOpening(it["vals"][j], [int.from_bytes(x, "little") for x in it["blinds"][j]])
                         for j in range(it["m"])])
    return [bytes(c) for c in comms], O.prove_with_rng(it["state"].clone(), ost, ow, M.ByteStreamRng(it["ext"])).to_bytes()


def _marshal(bpp, params, items, comms=None):
    """the bpp_prove_item array of `items`; comms[i]: the commitments item i brings, None (or comms = None): it brings none"""
    mar = bpp.RangeProof._openings_marshal([x["tr"] for x in items], [x["w"] for x in items], [x["mins"] for x in items],
                                           [x["nonce"] for x in items], [x["ext"] for x in items], params)
    _p, arr, n, keep = mar
    for i in range(n):
        if comms is not None and comms[i] is not None:
            buf = (ctypes.c_uint8 * (32 * items[i]["m"])).from_buffer_copy(b"".join(comms[i]))
            keep.append(buf)
            arr[i].commitments32 = ctypes.cast(buf, ctypes.c_void_p)
    return mar


def _openings(engine, mar, cstride=32 * M_MAX, sentinel=0xA5, commitments_out=True):
    """bpp_prove_openings into buffers filled with `sentinel` -> (rc, commitment slots, proofs, statuses, lengths, message)"""
    params, arr, n, _keep = mar
    out = (ctypes.c_uint8 * (STRIDE * n))(*([sentinel] * (STRIDE * n)))
    cs = (ctypes.c_uint8 * max(cstride * n, 1))(*([sentinel] * max(cstride * n, 1)))
    lens = (ctypes.c_size_t * n)()
    status = (ctypes.c_int * n)()
    err = ctypes.create_string_buffer(256)
    rc = engine.lib.bpp_prove_openings(engine.ctx, params.handle, arr, n, cs if commitments_out else None, cstride, out, STRIDE, lens,
                                       status, err, 256)
    raw, craw = bytes(out), bytes(cs)
    return (rc, [craw[i * cstride:(i + 1) * cstride] for i in range(n)], [raw[i * STRIDE:i * STRIDE + lens[i]] for i in range(n)],
            list(status), list(lens), err.value.decode())


def _mixed(engine, mar):
    """bpp_prove_batch_mixed -> (rc, proofs, statuses, lengths, message)"""
    params, arr, n, _keep = mar
    out = (ctypes.c_uint8 * (STRIDE * n))(*([0xA5] * (STRIDE * n)))
    lens = (ctypes.c_size_t * n)()
    status = (ctypes.c_int * n)()
    err = ctypes.create_string_buffer(256)
    rc = engine.lib.bpp_prove_batch_mixed(engine.ctx, params.handle, arr, n, out, STRIDE, lens, status, err, 256)
    raw = bytes(out)
    return rc, [raw[i * STRIDE:i * STRIDE + lens[i]] for i in range(n)], list(status), list(lens), err.value.decode()


def _uniform(engine, mar):
    params, arr, n, _keep = mar
    out = (ctypes.c_uint8 * (STRIDE * n))()
    plen = ctypes.c_size_t()
    err = ctypes.create_string_buffer(256)
    rc = engine.lib.bpp_prove_batch(engine.ctx, params.handle, arr, n, out, STRIDE, ctypes.byref(plen), err, 256)
    raw = bytes(out)
    return rc, [raw[i * STRIDE:i * STRIDE + plen.value] for i in range(n)], err.value.decode()


def _slot(it, comms):
    """what a successful item's slot of commitments_out holds: its 32 m bytes, the rest of the slot untouched"""
    return b"".join(comms) + bytes([0xA5]) * (32 * (M_MAX - it["m"]))


def _no_secrets_left(engine):
    examined, nonzero = ctypes.c_uint64(), ctypes.c_uint64()
    assert engine.lib.bpp_prove_secret_bytes(engine.ctx, ctypes.byref(examined), ctypes.byref(nonzero)) == 0
    assert examined.value > 0 and nonzero.value == 0


def _delta(before, after):
    return {k: after[k] - before[k] for k in STATS}


def _two_call(bpp, engine, params, it):
    """bpp_pedersen_commit, then a one-item bpp_prove_batch on the item: (commitments, rc, proof, message)"""
    comms = params.commit_many(it["vals"], it["blinds"])
    rc, proofs, msg = _uniform(engine, _marshal(bpp, params, [it], [comms]))
    return comms, rc, proofs[0], msg


# ---------------------------------------------------------------- 1. bytes, across shapes
@pytest.mark.parametrize("t", [1, 3])
@pytest.mark.parametrize("m", [1, 2, 4, 8])
def test_bytes_equal_the_oracle_and_the_two_call_form(bpp, engine, opt, m, t):
    params = _params(bpp, engine, t)
    # with and without promises, on a label and -- every third item -- on a 203-byte transcript state; m = 1: also with seed nonces
    items = _items(bpp, t, [m] * 3, b"openings-%d-%d" % (m, t), promises=True, state_every=3 if m <= 2 else 0)
    items += _items(bpp, t, [m] * 2, b"openings-none-%d-%d" % (m, t), promises=False)
    if m > 2:  # (the state transcript's oracle is oracle.pyref: too slow for m > 2; held to bpp_prove_batch_mixed there)
        items += [dict(x, state=_state(), tr=bpp.Transcript.from_state(_state().strobe.to_bytes()))
                  for x in _items(bpp, t, [m], b"openings-state-%d-%d" % (m, t))]
    if m == 1:
        items += _items(bpp, t, [1] * 3, b"openings-nonce-%d" % t, nonces=True, state_every=3)
    cp = cport.Params(N, M_MAX, t)
    want = [_oracle(x, cp) if (x["state"] is None or m <= 2) else None for x in items]
    commits = [[cp.commit(x["vals"][j], x["blinds"][j]) for j in range(m)] for x in items]
    cp.close()
    mar = _marshal(bpp, params, items)
    filled = _marshal(bpp, params, items, commits)
    for ct in (0, 1, 2):
        opt("ct", ct)
        rc, slots, proofs, status, lens, msg = _openings(engine, mar)
        assert rc == 0 and not any(status), (ct, msg, status)
        rcm, mixed, stm, lensm, msgm = _mixed(engine, filled)
        assert rcm == 0 and not any(stm), (ct, msgm)
        assert lens == lensm
        for i, x in enumerate(items):
            assert slots[i] == _slot(x, commits[i]), "commitments of item %d differ from the oracle's commit under ct = %d" % (i, ct)
            if want[i] is not None:
                assert want[i][0] == [bytes(c) for c in commits[i]]
                assert proofs[i] == want[i][1], "proof %d differs from the oracle prover's under ct = %d" % (i, ct)
            assert proofs[i] == mixed[i], "proof %d differs from bpp_prove_batch_mixed's under ct = %d" % (i, ct)
    # the equality the entry point promises, literally: bpp_pedersen_commit, then a one-item bpp_prove_batch
    opt("ct", -1)
    rc, slots, proofs, status, lens, msg = _openings(engine, mar)
    assert rc == 0, msg
    for i in (0, len(items) - 1):
        comms, rc2, proof, msg2 = _two_call(bpp, engine, params, items[i])
        assert rc2 == 0, msg2
        assert slots[i] == _slot(items[i], comms) and proofs[i] == proof
    _no_secrets_left(engine)


# ---------------------------------------------------------------- 2. edge openings
def test_edge_openings(bpp, engine, opt):
    t = 3
    params = _params(bpp, engine, t)
    rng = Prng(b"openings-edges")
    r = lambda: sb(O.random_not_zero(rng))  # noqa: E731
    zero, top = sb(0), sb(L_ORDER - 1)
    cases = [
        (1, [0], [[r(), r(), r()]]),
        (1, [2 ** 64 - 1], [[r(), r(), r()]]),
        (1, [12345], [[zero, r(), r()]]),
        (1, [12345], [[top, top, top]]),
        (1, [0], [[zero, zero, zero]]),  # commit(0, 0): the identity
        (2, [0, 2 ** 64 - 1], [[zero, r(), top], [top, zero, r()]]),
        (4, [2 ** 64 - 1, 0, 1, 2 ** 63], [[r(), r(), r()], [zero, zero, zero], [top, r(), zero], [r(), top, r()]]),
    ]
    items = []
    for m, vals, blinds in cases:
        rounds = (N * m).bit_length() - 1
        items.append(_item(bpp, t, m, vals, blinds, [None] * m, None, rng.fill_bytes(32 * (rounds + 3))))
    mar = _marshal(bpp, params, items)
    for ct in (0, 1, 2):
        opt("ct", ct)
        rc, slots, proofs, status, lens, msg = _openings(engine, mar)
        for i, x in enumerate(items):
            # whatever the two-call path returns, the new call returns it
            comms, rc2, proof, msg2 = _two_call(bpp, engine, params, x)
            assert status[i] == rc2, (ct, i, status[i], rc2, msg2)
            if rc2 == 0:
                assert slots[i] == _slot(x, comms) and proofs[i] == proof, (ct, i)
            else:
                assert slots[i][:32 * x["m"]] == bytes(32 * x["m"]) and proofs[i] == bytes(lens[i]), (ct, i)
                err = ctypes.create_string_buffer(256)
                code = engine.lib.bpp_prove_openings_item_message(engine.ctx, params.handle, ctypes.byref(mar[1][i]), None, 32 * M_MAX, STRIDE,
                                                                  status[i], err, 256)
                assert code == rc2 and err.value.decode() == msg2
        firsts = [s for s in status if s]
        assert rc == (firsts[0] if firsts else 0)
    # the oracle on the edge values it takes (its commit and its prover)
    cp = cport.Params(N, M_MAX, t)
    opt("ct", -1)
    rc, slots, proofs, status, lens, msg = _openings(engine, mar)
    for i in (0, 1, 2, 3, 5):
        assert status[i] == 0
        comms, proof = _oracle(items[i], cp)
        assert slots[i] == _slot(items[i], comms) and proofs[i] == proof, i
    cp.close()
    _no_secrets_left(engine)


# ---------------------------------------------------------------- 3. one ragged call of both kinds, with failures
RAGGED = [4, 1, 2, 1, 8, 1, 2, 4, 1, 2, 1, 1]
BRINGS = {0, 3, 4, 6, 9, 10}  # the items that bring their commitments
WRONG, BELOW_PROMISE, NON_CANONICAL = 3, 5, 9  # a wrong commitment brought; a value below its promise; a blinding factor = l


def _ragged_case(bpp, engine):
    if "ragged" not in _CACHE:
        t = 2
        params = _params(bpp, engine, t)
        items = _items(bpp, t, RAGGED, b"openings-ragged", nonces=True)
        cp = cport.Params(N, M_MAX, t)
        want = [_oracle(x, cp) for x in items]
        cp.close()
        comms = [want[i][0] if i in BRINGS else None for i in range(len(items))]
        bad = list(items)
        wrong = list(comms)
        wrong[WRONG] = [want[WRONG + 2][0][0]]  # (somebody else's commitment)
        x = items[BELOW_PROMISE]
        bad[BELOW_PROMISE] = dict(x, mins=[x["vals"][0] + 1])
        x = items[NON_CANONICAL]
        bl = [list(b) for b in x["blinds"]]
        bl[1][0] = L_ORDER.to_bytes(32, "little")
        bad[NON_CANONICAL] = _item(bpp, t, x["m"], x["vals"], bl, x["mins"], x["nonce"], x["ext"])
        _CACHE["ragged"] = (params, items, want, comms, bad, wrong)
    return _CACHE["ragged"]


def test_ragged_call_of_both_kinds(bpp, engine):
    params, items, want, comms, bad, wrong = _ragged_case(bpp, engine)
    rc, slots, proofs, status, lens, msg = _openings(engine, _marshal(bpp, params, items, comms))
    assert rc == 0 and not any(status), msg
    for i, x in enumerate(items):
        assert slots[i] == _slot(x, want[i][0]) and proofs[i] == want[i][1], i
        # its one-item form
        rc1, s1, p1, st1, _l, msg1 = _openings(engine, _marshal(bpp, params, [x], [comms[i]]))
        assert rc1 == 0 and s1[0] == slots[i] and p1[0] == proofs[i], (i, msg1)
    # the same call with three bad items: each fails alone
    mar = _marshal(bpp, params, bad, wrong)
    rc, slots, proofs, status, lens, msg = _openings(engine, mar)
    filled = [c if c is not None else want[i][0] for i, c in enumerate(wrong)]
    rcm, mixed, stm, lensm, msgm = _mixed(engine, _marshal(bpp, params, bad, filled))
    assert (rc, msg, status, lens) == (rcm, msgm, stm, lensm)
    assert status[WRONG] == INVALID_ARGUMENT and msg == "Witness opening is invalid!"
    assert status[BELOW_PROMISE] == INVALID_ARGUMENT and status[NON_CANONICAL] == INVALID_ARGUMENT
    err = ctypes.create_string_buffer(256)
    for i, text in ((WRONG, "Witness opening is invalid!"), (BELOW_PROMISE, "Minimum value is larger than value"),
                    (NON_CANONICAL, "blinding factor is not canonical")):
        code = engine.lib.bpp_prove_openings_item_message(engine.ctx, params.handle, ctypes.byref(mar[1][i]), None, 32 * M_MAX, STRIDE,
                                                          status[i], err, 256)
        assert code == status[i] and err.value.decode() == text
    for i, x in enumerate(items):
        if i in (WRONG, BELOW_PROMISE, NON_CANONICAL):
            assert slots[i] == bytes(32 * x["m"]) + bytes([0xA5]) * (32 * (M_MAX - x["m"])), "failed slot %d is not zeroed" % i
            assert proofs[i] == bytes(lens[i]) and lens[i] > 0
        else:
            assert status[i] == 0 and slots[i] == _slot(x, want[i][0]) and proofs[i] == want[i][1] == mixed[i], i
    _no_secrets_left(engine)


# ---------------------------------------------------------------- 4. call-level errors
def test_call_level_errors(bpp, engine):
    params, items, want, comms, _bad, _wrong = _ragged_case(bpp, engine)
    mar = _marshal(bpp, params, items, comms)
    rc, slots, proofs, status, lens, msg = _openings(engine, mar, commitments_out=False)
    assert rc == INVALID_ARGUMENT and msg == "null argument"
    assert all(p == bytes([0xA5]) * len(p) for p in proofs) and not any(status)
    # a slot of 64 bytes: the items of m <= 2 succeed, every larger one fails alone
    rc, slots, proofs, status, lens, msg = _openings(engine, mar, cstride=64)
    for i, x in enumerate(items):
        if x["m"] > 2:
            assert status[i] == INVALID_LENGTH and proofs[i] == bytes(lens[i])
            assert slots[i] == bytes([0xA5]) * 64, "a slot that is too small was written to"
        else:
            assert status[i] == 0 and proofs[i] == want[i][1] and slots[i] == (b"".join(want[i][0]) + bytes([0xA5]) * 64)[:64]
    assert rc == INVALID_LENGTH and msg == "commit_stride too small"
    err = ctypes.create_string_buffer(256)
    code = engine.lib.bpp_prove_openings_item_message(engine.ctx, params.handle, ctypes.byref(mar[1][0]), None, 64, STRIDE, INVALID_LENGTH, err, 256)
    assert code == INVALID_LENGTH and err.value == b"commit_stride too small"


# ---------------------------------------------------------------- 5. round trip through the verifier
def test_round_trip_through_the_verifier(bpp, engine):
    t = 2
    params = _params(bpp, engine, t)
    items = _items(bpp, t, [1, 4, 1, 2, 8, 1, 2, 1], b"openings-round-trip", nonces=True)
    args = ([x["tr"] for x in items], [x["w"] for x in items], [x["mins"] for x in items], [x["nonce"] for x in items],
            [x["ext"] for x in items], params)
    sts, proofs = bpp.RangeProof.prove_openings(*args)
    assert all(isinstance(s, bpp.RangeStatement) for s in sts) and all(isinstance(p, bpp.RangeProof) for p in proofs)
    for x, s in zip(items, sts):
        assert s.commitments_compressed == params.commit_many(x["vals"], x["blinds"])
    trs = [bpp.Transcript.new(LABEL)] * len(items)
    public = [bpp.RangeStatement.init(params, s.commitments_compressed, s.minimum_value_promises, None) for s in sts]
    assert bpp.RangeProof.verify_batch(trs, public, proofs, bpp.VerifyAction.VerifyOnly) == [None] * len(items)
    masks = bpp.RangeProof.verify_batch(trs, sts, proofs, bpp.VerifyAction.RecoverAndVerify)
    for x, mask in zip(items, masks):
        if x["nonce"] is None:
            assert mask is None
        else:
            assert mask.blindings() == x["blinds"][0]
    # the array form
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    np = importlib.import_module("numpy")
    sel = [x for x in items if x["m"] == 1]
    values = np.array([x["vals"] for x in sel], dtype=np.uint64)
    blindings = np.frombuffer(b"".join(b"".join(b"".join(r) for r in x["blinds"]) for x in sel), dtype=np.uint8).reshape(len(sel), 1, t, 32)
    mv = np.array([[v or 0 for v in x["mins"]] for x in sel], dtype=np.uint64)
    mp = np.array([[v is not None for v in x["mins"]] for x in sel], dtype=np.uint8)
    seeds = np.frombuffer(b"".join(x["nonce"] for x in sel), dtype=np.uint8).reshape(len(sel), 32)
    ext = np.frombuffer(b"".join(x["ext"] for x in sel), dtype=np.uint8).reshape(len(sel), -1)
    made, out = packed.prove(params, values, blindings, None, mv, mp, seeds, LABEL, ext)
    brought = packed.prove(params, values, blindings, made, mv, mp, seeds, LABEL, ext)
    assert out.tobytes() == brought.tobytes()
    assert [bytes(made[i, 0]) for i in range(len(sel))] == [s.commitments_compressed[0] for x, s in zip(items, sts) if x["m"] == 1]


# ---------------------------------------------------------------- 6. the pool
def test_pool_serves_both_kinds(bpp, engine):
    params, items, want, comms, _bad, _wrong = _ragged_case(bpp, engine)
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    pool = packed.ProvePool(params, lanes=2, max_wait_us=500)
    errors = []
    barrier = threading.Barrier(8)
    own = {i: _marshal(bpp, params, [items[i]], [want[i][0]]) for i in range(len(items))}
    bare = {i: _marshal(bpp, params, [items[i]]) for i in range(len(items))}
    direct = {i: _openings(engine, bare[i]) for i in range(len(items))}

    def worker(w):
        r = random.Random(w)
        barrier.wait()
        for _ in range(8):
            i = r.randrange(len(items))
            try:
                if (w + i) % 2:  # the existing kind: commitments brought, through bpp_prove_pool_prove
                    got = pool.prove_marshalled(own[i])
                    if got != [want[i][1]]:
                        errors.append((w, i, "bpp_prove_pool_prove: bytes differ"))
                else:
                    cs, got = pool.prove_openings_marshalled(bare[i])
                    if got != [want[i][1]] or cs != [want[i][0]] or got != direct[i][2] or b"".join(cs[0]) != direct[i][1][0][:32 * items[i]["m"]]:
                        errors.append((w, i, "bpp_prove_pool_openings: bytes differ"))
            except Exception as e:  # noqa: BLE001 (recorded, the test fails below)
                errors.append((w, i, repr(e)))

    ts = [threading.Thread(target=worker, args=(w,)) for w in range(8)]
    for th in ts:
        th.start()
    for th in ts:
        th.join()
    st, ost = pool.stats(), pool.openings_stats()
    # the pool hands on a failure as the direct call reports it: same code, same message
    x = items[BELOW_PROMISE]
    refused = _marshal(bpp, params, [dict(x, mins=[x["vals"][0] + 1])])
    rc, _s, _p, _st, _l, msg = _openings(engine, refused)
    with pytest.raises(bpp.ProofError) as e:
        pool.prove_openings_marshalled(refused)
    assert (int(e.value.kind), e.value.msg) == (rc, msg)
    # and still refuses an item without commitments that comes through the existing call
    with pytest.raises(bpp.ProofError) as e:
        pool.prove_marshalled(bare[1])
    assert (int(e.value.kind), e.value.msg) == (INVALID_ARGUMENT, "null witness / statement field")
    pool.close()
    assert not errors, errors[:3]
    assert st["pooled_calls"] + st["solo_calls"] == 64 and st["largest_calls"] > 1, st
    assert 0 < ost["openings_calls"] < 64 and ost["both_kinds_calls"] > 0, ost
    _no_secrets_left(engine)


# ---------------------------------------------------------------- 7. self-check on
def _tamper(opt, k, times, nonce=False, byte=40):
    opt("prove_check_tamper", k + 1)
    opt("prove_check_tamper_nonce", 1 if nonce else 0)
    opt("prove_check_tamper_byte", 0 if nonce else byte)
    opt("prove_check_tamper_xor", 0x10)
    opt("prove_check_tamper_times", times)


@pytest.mark.parametrize("nonce", [False, True])
@pytest.mark.parametrize("times", [1, 2])
def test_self_check_on_made_commitments(bpp, engine, opt, times, nonce):
    params, items, want, comms, _bad, _wrong = _ragged_case(bpp, engine)
    mar = _marshal(bpp, params, items, comms)
    opt("prove_check", 1)
    if nonce:
        opt("prove_check_recovery", 1)
    n_nonce = sum(1 for x in items if x["nonce"] is not None)
    s0, r0 = engine.prove_check_stats(), engine.prove_check_recovery_stats()
    rc, slots, proofs, status, lens, msg = _openings(engine, mar)
    assert rc == 0 and not any(status), msg
    assert [(s, p) for s, p in zip(slots, proofs)] == [(_slot(x, want[i][0]), want[i][1]) for i, x in enumerate(items)]
    assert _delta(s0, engine.prove_check_stats()) == dict(calls=1, proofs=len(items), batch_failures=0, remade=0, failed=0)
    r1 = engine.prove_check_recovery_stats()
    assert (r1["replayed"] - r0["replayed"], r1["mismatched"] - r0["mismatched"]) == (n_nonce if nonce else 0, 0)
    k = 5  # an m = 1 item with a seed nonce that brings no commitments
    assert k not in BRINGS and items[k]["nonce"] is not None
    _tamper(opt, k, times, nonce)
    s0 = engine.prove_check_stats()
    rc, slots, proofs, status, lens, msg = _openings(engine, mar)
    d = _delta(s0, engine.prove_check_stats())
    if times == 1:  # made again once, with correct bytes
        assert rc == 0 and not any(status), msg
        assert d == dict(calls=1, proofs=len(items), batch_failures=1, remade=1, failed=0)
    else:  # that item alone fails
        assert rc == SELF_CHECK and status == [SELF_CHECK if i == k else 0 for i in range(len(items))]
        assert "self-check" in msg and ("mask recovery" in msg) == nonce, msg
        assert d == dict(calls=1, proofs=len(items), batch_failures=1, remade=1, failed=1)
        assert slots[k] == bytes(32) + bytes([0xA5]) * (32 * (M_MAX - 1)) and proofs[k] == bytes(lens[k])
        # the message lookup knows the item by the commitment the engine made for it
        err = ctypes.create_string_buffer(256)
        first = (ctypes.c_uint8 * 32).from_buffer_copy(want[k][0][0])
        code = engine.lib.bpp_prove_openings_item_message(engine.ctx, params.handle, ctypes.byref(mar[1][k]), first, 32 * M_MAX, STRIDE,
                                                          status[k], err, 256)
        assert code == SELF_CHECK and err.value.decode() == msg
    for i, x in enumerate(items):
        if i != k or times == 1:
            assert slots[i] == _slot(x, want[i][0]) and proofs[i] == want[i][1], i
    _no_secrets_left(engine)
    # the knobs acted on that call only
    rc, slots, proofs, status, lens, msg = _openings(engine, mar)
    assert rc == 0 and proofs == [w[1] for w in want], msg


def test_self_check_failure_through_the_object_interface(bpp, engine, opt):
    params, items, want, _comms, _bad, _wrong = _ragged_case(bpp, engine)
    opt("prove_check", 1)
    opt("prove_check_recovery", 1)
    _tamper(opt, 5, 2, nonce=True)
    sts, res = bpp.RangeProof.prove_openings([x["tr"] for x in items], [x["w"] for x in items], [x["mins"] for x in items],
                                             [x["nonce"] for x in items], [x["ext"] for x in items], params)
    for i, (s, p) in enumerate(zip(sts, res)):
        if i == 5:
            assert isinstance(p, bpp.EngineError) and p is s and p.code == SELF_CHECK and "mask recovery" in str(p), p
        else:
            assert s.commitments_compressed == want[i][0] and p.to_bytes() == want[i][1]


# ---------------------------------------------------------------- 8. secret bytes
def test_no_secret_bytes_on_any_exit_path(bpp, engine):
    params, items, want, comms, bad, wrong = _ragged_case(bpp, engine)
    rc, *_ = _openings(engine, _marshal(bpp, params, items))  # every item from its openings alone
    assert rc == 0
    _no_secrets_left(engine)
    rc, *_ = _openings(engine, _marshal(bpp, params, bad, wrong))  # a call with failed items (host- and device-side)
    assert rc == INVALID_ARGUMENT
    _no_secrets_left(engine)
    rc, *_ = _openings(engine, _marshal(bpp, params, items), commitments_out=False)  # a call-level error
    assert rc == INVALID_ARGUMENT
    _no_secrets_left(engine)
    rc, *_ = _openings(engine, _marshal(bpp, params, items), cstride=0)  # every item refused on the host
    assert rc == INVALID_LENGTH
    _no_secrets_left(engine)


# ---------------------------------------------------------------- 9. the existing entry points are unchanged
def test_existing_entry_points_still_refuse_an_item_without_commitments(bpp, engine):
    params, items, want, comms, _bad, _wrong = _ragged_case(bpp, engine)
    text = "null witness / statement field"
    one = _marshal(bpp, params, [items[1]])
    rc, _proofs, msg = _uniform(engine, one)
    assert (rc, msg) == (INVALID_ARGUMENT, text)
    some = list(comms)
    mar = _marshal(bpp, params, items, some)
    rc, proofs, status, lens, msg = _mixed(engine, mar)
    assert (rc, msg) == (INVALID_ARGUMENT, text)
    for i in range(len(items)):
        if i in BRINGS:
            assert status[i] == 0 and proofs[i] == want[i][1]
        else:
            assert status[i] == INVALID_ARGUMENT and proofs[i] == bytes(lens[i])
            err = ctypes.create_string_buffer(256)
            assert engine.lib.bpp_prove_item_message(engine.ctx, params.handle, ctypes.byref(mar[1][i]), STRIDE, status[i], err, 256) == INVALID_ARGUMENT
            assert err.value.decode() == text
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    pool = packed.ProvePool(params, lanes=1)
    with pytest.raises(bpp.ProofError) as e:
        pool.prove_marshalled(one)
    pool.close()
    assert (int(e.value.kind), e.value.msg) == (INVALID_ARGUMENT, text)
