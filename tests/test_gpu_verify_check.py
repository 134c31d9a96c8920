"""GPU tests of the verifier's recheck ("verify_check" = 1): a rejection found on the device (tiers PASS1, PASS2, MSM) is verified
again under the complementary kernel forms with the plain MSM (csrc/msm_plain.h), a third time under the first forms when the two
disagree, and the outcome two passes share is returned (include/bpp.h, "Rechecked rejections").

Proofs are made by the engine's prover over 8-bit parameters (m = 1 with seed nonces, and m = 2 in an m_max = 2 set).  One
resident batch of 133 proofs is cut into groups of 1, 3, 64 and 65 -- a lone proof, a few, one whole wavefront of proofs, one more
than that -- and, as the chunked form, into 50 + 50 + 33.  The three kinds of invalid proof are one per device tier: one bit of r1
changed (the final MSM), an A whose encoding has bit 0 set (no ristretto255 point: decompression, PASS 2), an all-zero A1 (the
identity: PASS 1).  The test knobs "verify_check_tamper*" alter bytes of page-locked host memory behind a pass; nothing on the device
is made to fault."""
import ctypes
import importlib

import numpy as np
import pytest

from oracle import cport
from oracle.pyref import protocol as O
from tests.helpers import LABEL, Prng, sb

pytestmark = pytest.mark.gpu

N_BITS, T = 8, 1
BOUNDS = [0, 1, 4, 68, 133]
TOTAL = BOUNDS[-1]
VERIFY_ONLY, RECOVER_AND_VERIFY = 0, 1
TIER_PASS1, TIER_PASS2, TIER_MSM, TIER_ENGINE = 5, 6, 7, 255
SELF_CHECK = -5
STATS = ("calls", "rechecked_groups", "confirmed", "overturned", "tie_breaks", "undecided")
OFF_A, OFF_A1, OFF_R1 = 1 + 32 * T, 1 + 32 * (T + 1), 1 + 32 * (T + 3)
_CACHE = {}


def _packed():
    return importlib.import_module("bulletproofs-plus_amd.packed")


def _case(bpp, engine, m):
    """TOTAL valid proofs of aggregation m made by the engine's prover, as arrays (made once, never altered)"""
    if m not in _CACHE:
        P = _packed()
        params = bpp.RangeParameters.init(N_BITS, m, bpp.create_pedersen_gens_with_extension_degree(T), engine=engine)
        n = TOTAL if m == 1 else 7
        rng = Prng(b"verify-check-%d" % m)
        rounds = (N_BITS * m).bit_length() - 1
        values = np.array([[rng.next_u64() % (1 << (N_BITS - 1)) for _ in range(m)] for _ in range(n)], dtype=np.uint64)
        blind = np.frombuffer(b"".join(sb(O.random_not_zero(rng)) for _ in range(n * m * T)), dtype=np.uint8).reshape(n, m, T, 32).copy()
        mins = values // 3
        present = np.ones((n, m), dtype=np.uint8)
        seeds = np.frombuffer(b"".join(sb(O.random_not_zero(rng)) for _ in range(n)), dtype=np.uint8).reshape(n, 32).copy() if m == 1 else None
        ext = np.frombuffer(rng.fill_bytes(n * 32 * (rounds + 3)), dtype=np.uint8).reshape(n, -1).copy()
        comms = P.commit(params, values.reshape(-1), blind.reshape(n * m, T, 32)).reshape(n, m, 32)
        proofs = P.prove(params, values, blind, comms, mins, present, seeds, LABEL, ext)
        _CACHE[m] = dict(params=params, n=n, m=m, proofs=proofs, comms=comms, mins=mins, present=present, seeds=seeds, blind=blind)
    return _CACHE[m]


def _spoil(proofs, index, kind):
    """a copy of the proofs with proof `index` made invalid"""
    p = proofs.copy()
    if kind == "msm":
        p[index, OFF_R1] ^= 1          # one bit of r1: still canonical, the final check fails
    elif kind == "decode":
        p[index, OFF_A] |= 1           # a negative s: no ristretto255 encoding
    elif kind == "identity":
        p[index, OFF_A1:OFF_A1 + 32] = 0  # the identity: refused when it is appended to the transcript
    else:
        raise AssertionError(kind)
    return p


EXPECT = {"msm": (1, TIER_MSM), "decode": (2, TIER_PASS2), "identity": (1, TIER_PASS1)}


def _resident(c, proofs):
    return _packed().ResidentBatch(c["params"], proofs, c["comms"], c["mins"], c["present"], c["seeds"], LABEL)


def _groups(rb, actions=None):
    res, masks, present = _packed().verify_groups_actions(rb, BOUNDS, actions or [RECOVER_AND_VERIFY] * (len(BOUNDS) - 1))
    return res, masks.tobytes(), present.tobytes()


def _chunked(engine, rb, action, chunk):
    masks = np.full((rb.n, T, 32), 0xA5, dtype=np.uint8)
    present = np.full(rb.n, 0xA5, dtype=np.uint8)
    err = ctypes.create_string_buffer(256)
    rc = engine.lib.bpp_verify_resident(engine.ctx, rb.handle, action, chunk, masks.ctypes.data, present.ctypes.data, err, 256)
    return rc, err.value, masks.tobytes(), present.tobytes()


def _delta(engine, before):
    after = engine.verify_check_stats()
    return {k: after[k] - before[k] for k in STATS}


def _counts(**kw):
    d = dict.fromkeys(STATS, 0)
    d.update(kw)
    return d


def _want_masks(c, ok_groups):
    """what RecoverAndVerify returns: the witness's blinding factors for the proofs of the groups that verify, zero elsewhere"""
    masks = np.zeros((c["n"], T, 32), dtype=np.uint8)
    present = np.zeros(c["n"], dtype=np.uint8)
    for g in ok_groups:
        lo, hi = BOUNDS[g], BOUNDS[g + 1]
        masks[lo:hi] = c["blind"][lo:hi, 0]
        present[lo:hi] = 1
    return masks.tobytes(), present.tobytes()


def _plan(rb):
    return rb.trace(7)


# (kind of invalid proof, group, position inside the group): every group size and every tier once, the last proof of the
# 65-proof group (the second wavefront of its terms) among them
PLACES = [("msm", 3, 64), ("decode", 2, 5), ("identity", 1, 2), ("msm", 0, 0), ("decode", 3, 0)]


@pytest.mark.parametrize("kind,group,pos", PLACES)
def test_confirmed_rejection_equals_the_unchecked_call(bpp, engine, opt, kind, group, pos):
    c = _case(bpp, engine, 1)
    rb = _resident(c, _spoil(c["proofs"], BOUNDS[group] + pos, kind))
    try:
        off = _groups(rb)
        plan = _plan(rb)
        code, tier = EXPECT[kind]
        for g, r in enumerate(off[0]):
            want = (code, tier, 0 if kind == "msm" else pos) if g == group else (0, 0, 0)  # (the final check names no proof)
            assert (r["code"], r["tier"], r["index"]) == want, (g, r)
        assert off[1:] == _want_masks(c, [g for g in range(4) if g != group])
        opt("verify_check", 1)
        s0 = engine.verify_check_stats()
        on = _groups(rb)
        assert on == off  # code, tier, index, message, masks, zeroed mask slots
        assert _delta(engine, s0) == _counts(calls=1, rechecked_groups=1, confirmed=1)
        assert _plan(rb) == plan, "BPP_TRACE_PLAN changed over a rechecked call"
        assert _groups(rb) == off  # and the batch verifies as before afterwards
        opt("verify_check", 0)
        assert _groups(rb) == off
    finally:
        rb.close()


@pytest.mark.parametrize("kind", ["msm", "decode", "identity"])
def test_chunked_form_with_a_ragged_last_chunk(bpp, engine, opt, kind):
    c = _case(bpp, engine, 1)
    rb = _resident(c, _spoil(c["proofs"], 120, kind))  # in the last chunk of 50 + 50 + 33
    try:
        off = _chunked(engine, rb, RECOVER_AND_VERIFY, 50)
        assert off[0] == EXPECT[kind][0]
        opt("verify_check", 1)
        s0 = engine.verify_check_stats()
        assert _chunked(engine, rb, RECOVER_AND_VERIFY, 50) == off
        assert _delta(engine, s0) == _counts(calls=1, rechecked_groups=1, confirmed=1)
        assert _chunked(engine, rb, VERIFY_ONLY, 0)[:2] == _chunked(engine, rb, VERIFY_ONLY, 50)[:2] == off[:2]
    finally:
        rb.close()


def test_valid_input_counts_calls_only(bpp, engine, opt):
    c = _case(bpp, engine, 1)
    rb = _resident(c, c["proofs"])
    try:
        off = _groups(rb)
        assert all(r["code"] == 0 for r in off[0]) and off[1:] == _want_masks(c, range(4))
        opt("verify_check", 1)
        s0 = engine.verify_check_stats()
        assert _groups(rb) == off
        rc, _, masks, present = _chunked(engine, rb, RECOVER_AND_VERIFY, 50)
        assert rc == 0 and (masks, present) == _want_masks(c, range(4))
        assert _delta(engine, s0) == _counts(calls=2)
    finally:
        rb.close()


@pytest.mark.parametrize("bad", [None, 3])
def test_aggregated_proofs_and_the_oracle(bpp, engine, opt, bad):
    """m = 2 in an m_max = 2 set through bpp_verify_batch_packed; the rejected batch also through the CPU oracle"""
    c = _case(bpp, engine, 2)
    P = _packed()
    proofs = c["proofs"] if bad is None else _spoil(c["proofs"], bad, "msm")
    inp = P.PackedInput(proofs, c["comms"], c["mins"], c["present"], None, LABEL)

    def call():
        err = ctypes.create_string_buffer(256)
        rc = engine.lib.bpp_verify_batch_packed(engine.ctx, c["params"].handle, ctypes.byref(inp.struct), VERIFY_ONLY, 0, None, None, err, 256)
        return rc, err.value

    off = call()
    opt("verify_check", 1)
    s0 = engine.verify_check_stats()
    assert call() == off
    cp = cport.Params(N_BITS, 2, T)
    rc, _, _ = cp.verify([dict(proof=proofs[i].tobytes(), commitments=[c["comms"][i, j].tobytes() for j in range(2)],
                               min_values=[int(v) for v in c["mins"][i]], seed_nonce=None, label=LABEL) for i in range(c["n"])])
    cp.close()
    assert off[0] == rc == (0 if bad is None else 1)
    assert _delta(engine, s0) == (_counts(calls=1) if bad is None else _counts(calls=1, rechecked_groups=1, confirmed=1))


@pytest.mark.parametrize("kind,tier,code", [(1, TIER_MSM, 1), (3, TIER_PASS1, 1), (4, TIER_PASS2, 2)])
@pytest.mark.parametrize("group", [1, 3])
def test_false_rejection_in_pass_one_is_overturned(bpp, engine, opt, kind, tier, code, group):
    c = _case(bpp, engine, 1)
    rb = _resident(c, c["proofs"])
    try:
        clean = _groups(rb)
        plan = _plan(rb)

        def tamper(passes):
            opt("verify_check_tamper", passes)
            opt("verify_check_tamper_group", group)
            opt("verify_check_tamper_kind", kind)

        tamper(1)
        off = _groups(rb)  # the unchecked engine returns the false rejection
        r = off[0][group]
        assert (r["code"], r["tier"], r["index"]) == (code, tier, 0)
        assert off[1:] == _want_masks(c, [g for g in range(4) if g != group])
        assert _groups(rb) == clean  # the knobs acted on that call only
        opt("verify_check", 1)
        tamper(1)
        s0 = engine.verify_check_stats()
        assert _groups(rb) == clean  # Ok, with the right masks
        assert _delta(engine, s0) == _counts(calls=1, rechecked_groups=1, overturned=1, tie_breaks=1)
        assert _plan(rb) == plan
        # passes 1 and 3 altered: two of three say "rejected", and that is returned
        tamper(1 | 4)
        s0 = engine.verify_check_stats()
        assert _groups(rb) == off
        assert _delta(engine, s0) == _counts(calls=1, rechecked_groups=1, confirmed=1, tie_breaks=1)
    finally:
        rb.close()


def test_false_acceptance_in_pass_two_does_not_save_an_invalid_group(bpp, engine, opt):
    c = _case(bpp, engine, 1)
    for kind in ("msm", "decode"):
        rb = _resident(c, _spoil(c["proofs"], BOUNDS[2] + 63, kind))
        try:
            off = _groups(rb)
            opt("verify_check", 1)
            opt("verify_check_tamper", 2)
            opt("verify_check_tamper_group", 2)
            opt("verify_check_tamper_kind", 2)
            s0 = engine.verify_check_stats()
            assert _groups(rb) == off  # still rejected
            assert _delta(engine, s0) == _counts(calls=1, rechecked_groups=1, confirmed=1, tie_breaks=1)
            opt("verify_check", 0)
        finally:
            rb.close()


def test_three_different_outcomes_are_a_self_check_failure(bpp, engine, opt):
    c = _case(bpp, engine, 1)
    rb = _resident(c, _spoil(c["proofs"], BOUNDS[1] + 1, "msm"))
    try:
        off = _groups(rb)
        opt("verify_check", 1)
        opt("verify_check_tamper", 2 | 4)
        opt("verify_check_tamper_group", 1)
        opt("verify_check_tamper_kind", (3 << 4) | (4 << 8))  # pass 2: a PASS-1 finding, pass 3: a decompression finding
        s0 = engine.verify_check_stats()
        res, masks, present = _groups(rb)
        assert _delta(engine, s0) == _counts(calls=1, rechecked_groups=1, tie_breaks=1, undecided=1)
        r = res[1]
        assert (r["code"], r["tier"]) == (SELF_CHECK, TIER_ENGINE)
        for outcome in ("1/7/0", "1/5/0", "2/6/0"):
            assert outcome in r["msg"], r["msg"]
        assert [x for g, x in enumerate(res) if g != 1] == [x for g, x in enumerate(off[0]) if g != 1]
        assert (masks, present) == off[1:]  # the undecided group gets no masks, the others theirs
        # the chunked form returns the engine fault as its code
        opt("verify_check_tamper", 2 | 4)
        opt("verify_check_tamper_group", 0)
        opt("verify_check_tamper_kind", (3 << 4) | (4 << 8))
        rc, msg, _, _ = _chunked(engine, rb, VERIFY_ONLY, 0)
        assert rc == SELF_CHECK and b"three passes" in msg
    finally:
        rb.close()


def test_pipeline_lanes_recheck(bpp, engine, opt):
    """bpp_verify_submit_packed / bpp_verify_collect: the lanes copy the option when they are made, the context's counters add theirs"""
    c = _case(bpp, engine, 1)
    P = _packed()
    eng = bpp.Engine(0)
    try:
        params = c["params"].share(eng)
        pipe = P.Pipeline(params, depth=2)
        bad = P.PackedInput(_spoil(c["proofs"], 70, "decode")[:100], c["comms"][:100], c["mins"][:100], c["present"][:100], c["seeds"][:100], LABEL)
        good = P.PackedInput(c["proofs"][:100], c["comms"][:100], c["mins"][:100], c["present"][:100], c["seeds"][:100], LABEL)
        want_err = None
        try:
            P.verify_batch(params, bad, RECOVER_AND_VERIFY, chunk=40)
        except bpp.ProofError as e:
            want_err = (e.kind, str(e))
        assert want_err is not None and want_err[0] == bpp.ProofErrorKind.InvalidArgument
        want_masks = P.verify_batch(params, good, RECOVER_AND_VERIFY, chunk=40)
        eng.set_option("verify_check", 1)  # before the first submit
        s0 = eng.verify_check_stats()
        tickets = [pipe.submit(x, RECOVER_AND_VERIFY, chunk=40) for x in (bad, good, bad)]
        got = []
        for t in tickets:
            try:
                m, p = pipe.collect(t)
                got.append((m.tobytes(), p.tobytes()))
            except bpp.ProofError as e:
                got.append((e.kind, str(e)))
        assert got == [want_err, (want_masks[0].tobytes(), want_masks[1].tobytes()), want_err]
        after = eng.verify_check_stats()
        assert {k: after[k] - s0[k] for k in STATS} == _counts(calls=3, rechecked_groups=2, confirmed=2)
    finally:
        eng.close()


def test_batcher_lanes_recheck(bpp, engine, opt):
    c = _case(bpp, engine, 1)
    P = _packed()
    lib = engine.lib
    bad = P.PackedInput(_spoil(c["proofs"], 2, "identity")[:5], c["comms"][:5], c["mins"][:5], c["present"][:5], c["seeds"][:5], LABEL)
    good = P.PackedInput(c["proofs"][5:70], c["comms"][5:70], c["mins"][5:70], c["present"][5:70], c["seeds"][5:70], LABEL)
    opt("verify_check", 1)  # before the batcher is made: its lanes copy the option
    b = P.Batcher(c["params"], good, lanes=2)
    try:
        s0 = _lib_stats(bpp, lib, b)
        with pytest.raises(bpp.ProofError) as e:
            b.verify_action(bad, RECOVER_AND_VERIFY)
        assert e.value.kind == bpp.ProofErrorKind.VerificationFailed and "Identity element" in str(e.value)
        masks, present = b.verify_action(good, RECOVER_AND_VERIFY)
        assert masks.tobytes() == c["blind"][5:70, 0].tobytes() and present.tobytes() == bytes([1]) * 65
        # a false rejection on the batcher's first lane (the context it was made from) is overturned
        opt("verify_check_tamper", 1)
        opt("verify_check_tamper_group", 0)
        opt("verify_check_tamper_kind", 1)
        masks, present = b.verify_action(good, RECOVER_AND_VERIFY)
        assert masks.tobytes() == c["blind"][5:70, 0].tobytes() and present.tobytes() == bytes([1]) * 65
        s1 = _lib_stats(bpp, lib, b)
        assert {k: s1[k] - s0[k] for k in STATS} == _counts(calls=3, rechecked_groups=2, confirmed=1, overturned=1, tie_breaks=1)
    finally:
        b.close()


def _lib_stats(bpp, lib, batcher):
    s = bpp._lib.VerifyCheckStats()
    assert lib.bpp_batcher_verify_check_stats(batcher.handle, ctypes.byref(s)) == 0
    return {k: int(getattr(s, k)) for k in STATS}


def test_default_context_rechecks_nothing(bpp, engine):
    """the option is off by default: a rejection is returned after one pass and no counter moves"""
    c = _case(bpp, engine, 1)
    eng = bpp.Engine(0)
    try:
        params = c["params"].share(eng)
        bad = _packed().PackedInput(_spoil(c["proofs"], 1, "msm")[:3], c["comms"][:3], c["mins"][:3], c["present"][:3], c["seeds"][:3], LABEL)
        with pytest.raises(bpp.ProofError):
            _packed().verify_batch(params, bad, VERIFY_ONLY, chunk=0)
        assert eng.verify_check_stats() == _counts()
    finally:
        eng.close()


def test_prover_self_check_is_left_alone(bpp, engine, opt):
    """the checks of tests/test_gpu_prove_check.py hold with "verify_check" = 1 on the proving context: the self-check's own
    verifications run with the recheck off, its counts are what they were, and the recheck's counters do not move"""
    from tests import test_gpu_prove_check as PC
    opt("verify_check", 1)
    s0 = engine.verify_check_stats()
    PC.test_mixed_checked_equals_unchecked_and_counts_valid_items(bpp, engine, opt)
    for site, times in (("msm", 1), ("msm", 2), ("decompress", 2)):  # (the 8-bit mixed case: located, remade, failing alone)
        PC.test_mixed_tampered_proof(bpp, engine, opt, site, times)
    assert _delta(engine, s0) == _counts()
