"""GPU tests of the joint final check ("verify_joint" = 1, include/bpp.h "Joint final check"): a verification pass with two or more
groups, all held to the final check, runs ONE multiscalar multiplication over all of them -- the generator columns under the sum of
the groups' rows, every dynamic term with the scalar it has -- and the per-group ones only when that check fails.

Inputs: twelve non-aggregated 64-bit proofs (cols = 130, 16 dynamic terms per proof) made by the engine's prover with bench.py's
recipe; the first seven as ragged groups [0, 1, 3, 6, 7] through bpp_verify_resident_groups, all twelve as chunks of 5 + 5 + 2
through bpp_verify_resident.  Every comparison is exact: bytes, codes, tiers, indices, messages, counters.  The oracle is
oracle.pyref (verify() per group for the scalars, its point arithmetic for the sum of the groups' results)."""
import ctypes
import importlib
import threading

import numpy as np
import pytest

from oracle.pyref import curve as C
from oracle.pyref import protocol as O
from tests import helpers as H
from tests.helpers import LABEL, sb

pytestmark = pytest.mark.gpu

COLS, DYN = 130, 16
BOUNDS = [0, 1, 3, 6, 7]
VERIFY_ONLY, RECOVER_AND_VERIFY, RECOVER_ONLY = 0, 1, 2
OFF_A, OFF_R1 = 1 + 32, 1 + 32 + 96
STATS = ("calls", "accepted", "fallbacks", "fallback_all_ok")
ZERO = bytes(32)


@pytest.fixture(scope="module")
def packed():
    return importlib.import_module("bulletproofs-plus_amd.packed")


@pytest.fixture(scope="module")
def data(bpp, packed, engine):
    import bench
    params = bpp.RangeParameters.init(64, 1, bpp.create_pedersen_gens_with_extension_degree(1), engine=engine)
    d = bench.make_inputs(np, packed, params, 12, seed=20261019)
    yield params, d
    params.close()


def _rb(packed, data, n, proofs=None, seeds=False):
    params, d = data
    pr = d["proofs"] if proofs is None else proofs
    return packed.ResidentBatch(params, pr[:n], d["commitments"][:n], d["min_values"][:n], d["min_present"][:n],
                                d["seeds"][:n] if seeds else None, LABEL)


def _spoil(d, index, kind="r1"):
    p = d["proofs"].copy()
    if kind == "r1":
        p[index, OFF_R1 + 5] ^= 2  # one bit of r1: still canonical, only the final check notices
    else:
        p[index, OFF_A] |= 1       # a negative s: no ristretto255 encoding (decompression, InvalidArgument)
    return p


def _delta(engine, before):
    after = engine.verify_joint_stats()
    return {k: after[k] - before[k] for k in STATS}


def _counts(**kw):
    out = dict.fromkeys(STATS, 0)
    out.update(kw)
    return out


# the two forms of the issue's inputs: (proofs in the batch, run) with run(rb) -> something comparable that holds every result
def _run_groups(packed):
    def run(rb):
        return packed.verify_groups(rb, BOUNDS)
    return run


def _run_chunked(bpp):
    def run(rb):
        try:
            rb.verify_only(chunk=5)
            return (0, "")
        except bpp.ProofError as e:
            return (int(e.kind), str(e))
    return run


FORMS = {"groups": (7, [0, 1, 3, 6, 7]), "chunk5": (12, [0, 5, 10, 12])}


def _runner(form, bpp, packed):
    return _run_groups(packed) if form == "groups" else _run_chunked(bpp)


def _all_ok(form, res):
    return all(r["code"] == 0 and r["tier"] == 0 for r in res) if form == "groups" else res == (0, "")


def _oracle_group(d, lo, hi):
    o_params = O.RangeParameters(64, 1, O.PedersenGens(1))
    sts = [O.RangeStatement(o_params, [C.decompress(bytes(d["commitments"][i, 0]))], [int(d["min_values"][i, 0])], None) for i in range(lo, hi)]
    proofs = [O.RangeProof.from_bytes(bytes(d["proofs"][i])) for i in range(lo, hi)]
    case = H.Case()
    case.label = LABEL
    _, tr = H.oracle_verify_trace(case, statements=sts, proofs=proofs)
    return tr


@pytest.mark.parametrize("form", ["groups", "chunk5"])
def test_accepted(bpp, packed, engine, opt, data, form):
    n, bounds = FORMS[form]
    run = _runner(form, bpp, packed)
    rb = _rb(packed, data, n)
    try:
        off = run(rb)
        assert _all_ok(form, off)
        off_tr = [rb.trace(w) for w in (3, 4, 5)]
        assert rb.trace(6) == ZERO * (len(bounds) - 1)
        with pytest.raises(bpp.ProofError):
            rb.trace(8)  # no joint check ran
        opt("verify_joint", 1)
        s0 = engine.verify_joint_stats()
        on = run(rb)
        assert on == off
        assert _delta(engine, s0) == _counts(calls=1, accepted=1)
        plan = engine.msm_last_plan()
        ng = COLS + DYN * n
        assert rb.shape()["total_dyn"] == DYN * n and rb.shape()["groups"] == len(bounds) - 1
        assert plan["G"] == 1 and plan["terms"] == 2 * ng and plan["quad"], plan  # (a small call: the half-scalar plan, every term twice)
        assert rb.trace(8) == ZERO
        with pytest.raises(bpp.ProofError) as e:
            rb.trace(6)
        assert e.value.kind == bpp.ProofErrorKind.InvalidArgument and "joint" in str(e.value)
        assert [rb.trace(w) for w in (3, 4, 5)] == off_tr
        # ... and through them the oracle's, group by group: every group keeps the weights of its own chain
        d = data[1]
        for g in range(len(bounds) - 1):
            lo, hi = bounds[g], bounds[g + 1]
            tr = _oracle_group(d, lo, hi)
            assert off_tr[0][32 * lo:32 * hi] == b"".join(sb(w) for w in tr["weights"]), g
            static = b"".join(sb(a) + sb(b) for a, b in zip(tr["gi"], tr["hi"])) + b"".join(sb(x) for x in tr["g"]) + sb(tr["h"])
            assert off_tr[1][32 * COLS * g:32 * COLS * (g + 1)] == static, g
            assert off_tr[2][32 * DYN * lo:32 * DYN * hi] == b"".join(sb(x) for x in tr["dynamic_scalars"]), g
        opt("verify_joint", 0)
        assert run(rb) == off and rb.trace(6) == ZERO * (len(bounds) - 1)  # the per-group MSMs are back
    finally:
        rb.close()


@pytest.mark.parametrize("form,bad", [("groups", 0), ("groups", 4), ("groups", 6), ("chunk5", 2), ("chunk5", 7), ("chunk5", 11)])
def test_rejected_is_the_per_group_outcome(bpp, packed, engine, opt, data, form, bad):
    """one scalar byte of one proof flipped, in the first, a middle and the last group"""
    n, bounds = FORMS[form]
    run = _runner(form, bpp, packed)
    rb = _rb(packed, data, n, _spoil(data[1], bad))
    try:
        off = run(rb)
        assert not _all_ok(form, off)
        pts = rb.trace(6)
        bad_group = max(g for g in range(len(bounds) - 1) if bounds[g] <= bad)
        assert [pts[32 * g:32 * g + 32] != ZERO for g in range(len(bounds) - 1)] == [g == bad_group for g in range(len(bounds) - 1)]
        if form == "groups":
            r = off[bad_group]
            assert (r["code"], r["tier"], r["index"]) == (int(bpp.ProofErrorKind.VerificationFailed), 7, 0)
        opt("verify_joint", 1)
        s0 = engine.verify_joint_stats()
        assert run(rb) == off  # results, error kind, tier, index, message
        assert _delta(engine, s0) == _counts(calls=1, fallbacks=1)
        assert rb.trace(6) == pts  # it ran
        joint = rb.trace(8)
        acc = C.Point.identity()
        for g in range(len(bounds) - 1):
            acc = acc + C.decompress(pts[32 * g:32 * g + 32])
        assert joint != ZERO and joint == acc.compress()
        assert not engine.msm_last_plan()["G"] == 1  # the last MSM of the call was the per-group one
    finally:
        rb.close()


def test_two_bad_groups_with_different_findings(bpp, packed, engine, opt, data):
    d = data[1]
    p = _spoil(d, 2, "decode")
    p[6, OFF_R1 + 5] ^= 2
    rb = _rb(packed, data, 7, p)
    try:
        off = packed.verify_groups(rb, BOUNDS)
        K = bpp.ProofErrorKind
        assert [(r["code"], r["tier"], r["index"]) for r in off] == [(0, 0, 0), (int(K.InvalidArgument), 6, 1), (0, 0, 0), (int(K.VerificationFailed), 7, 0)]
        opt("verify_joint", 1)
        s0 = engine.verify_joint_stats()
        assert packed.verify_groups(rb, BOUNDS) == off
        assert _delta(engine, s0) == _counts(calls=1, fallbacks=1)
    finally:
        rb.close()


def test_forced_fallback_on_a_valid_input(bpp, packed, engine, opt, data):
    rb = _rb(packed, data, 7)
    try:
        off = packed.verify_groups(rb, BOUNDS)
        opt("verify_joint", 1)
        opt("verify_check_tamper", 1)
        opt("verify_check_tamper_kind", 5)
        s0 = engine.verify_joint_stats()
        assert packed.verify_groups(rb, BOUNDS) == off and _all_ok("groups", off)
        assert _delta(engine, s0) == _counts(calls=1, fallbacks=1, fallback_all_ok=1)
        assert rb.trace(8) == ZERO and rb.trace(6) == ZERO * 4
        s0 = engine.verify_joint_stats()
        assert packed.verify_groups(rb, BOUNDS) == off  # the knob acted on that call only
        assert _delta(engine, s0) == _counts(calls=1, accepted=1)
    finally:
        rb.close()


def test_recover_only_group_and_single_group_take_the_old_path(bpp, packed, engine, opt, data):
    rb = _rb(packed, data, 7, seeds=True)
    try:
        def mixed():
            res, masks, present = packed.verify_groups_actions(rb, BOUNDS, [RECOVER_AND_VERIFY, RECOVER_ONLY, VERIFY_ONLY, RECOVER_AND_VERIFY])
            return res, masks.tobytes(), present.tobytes()

        def single():
            rb.verify_only(chunk=0)
            return rb.trace(6)

        def all_recover():
            res, masks, present = packed.verify_groups_actions(rb, BOUNDS, [RECOVER_AND_VERIFY] * 4)
            return res, masks.tobytes(), present.tobytes()

        off = [mixed(), single(), all_recover()]
        assert off[0][2] == bytes([1, 1, 1, 0, 0, 0, 1]) and off[2][2] == bytes([1]) * 7
        assert off[2][1] == data[1]["blindings"][:7, 0, 0].tobytes()  # the witness's blinding factors
        opt("verify_joint", 1)
        s0 = engine.verify_joint_stats()
        assert mixed() == off[0] and single() == off[1]
        assert _delta(engine, s0) == _counts()
        assert all_recover() == off[2]  # RecoverAndVerify in every group: the joint path, the same masks
        assert _delta(engine, s0) == _counts(calls=1, accepted=1)
    finally:
        rb.close()


def test_sharded_form_with_two_ranks_stays_as_it_is(bpp, packed, engine, data):
    """bpp_verify_sharded_groups, two in-process ranks, two reference batches of three proofs sharded 2 + 1: the option is set on
    both ranks' contexts, the results are those without it and no joint check is counted"""
    dmod = importlib.import_module("bulletproofs-plus_amd.dist")
    params, d = data
    counts, world, G, n, first = [2, 1], 2, 2, 3, [0, 2]
    proofs = _spoil(d, 4)  # group 1, rank 0
    out = {}
    for joint in (0, 1):
        engs = [bpp.Engine(0) for _ in range(world)]
        pars = [params.share(e) for e in engs]
        comms = [dmod.ShardComm(engs[r], r, world, local_group=5150 + joint) for r in range(world)]
        for e in engs:
            e.set_option("verify_joint", joint)
        res = [None] * world

        def rank_main(r):
            idx = np.concatenate([np.arange(n * g + first[r], n * g + first[r] + counts[r]) for g in range(G)])
            rb = packed.ResidentBatch(pars[r], proofs[idx], d["commitments"][idx], d["min_values"][idx], d["min_present"][idx], None, LABEL)
            try:
                res[r] = [(x["code"], x["tier"], x["rank"], x["index"]) for x in comms[r].verify_groups(rb, G, counts)]
            except BaseException as e:  # noqa: BLE001
                res[r] = ("exception", repr(e))
            finally:
                rb.close()
        ths = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
        for t in ths:
            t.start()
        for t in ths:
            t.join(timeout=120)
        assert not any(t.is_alive() for t in ths), "a rank is stuck in a collective"
        out[joint] = (res, [e.verify_joint_stats() for e in engs])
        for c in comms:
            c.close()
        for p in pars:
            p.close()
        for e in engs:
            e.close()
    assert out[0][0][0] == out[0][0][1] == [(0, 0, -1, 0), (int(bpp.ProofErrorKind.VerificationFailed), 7, -1, 0)]
    assert out[1] == out[0] and out[1][1] == [_counts()] * world


@pytest.mark.parametrize("chain,zero", [(0, 0), (1, 0), (2, 0), (1, 2), (2, 2)])
def test_weight_chain_modes_and_the_redraw(bpp, packed, engine, opt, data, chain, zero):
    """a two-group call (3 + 3 proofs) with the chains on the host, on the device, and split; chain_test_zero makes the device report
    proof 1's weight as zero: the pass is repeated with the chains on the host and counts once (the host chains redraw by themselves)"""
    rb = _rb(packed, data, 6)
    try:
        opt("chain", chain)
        rb.verify_only(chunk=3)
        want = [rb.trace(w) for w in (3, 4, 5)]
        opt("verify_joint", 1)
        if zero:
            opt("chain_test_zero", zero)
        s0, c0 = engine.verify_joint_stats(), engine.device_chain_stats()
        rb.verify_only(chunk=3)
        assert _delta(engine, s0) == _counts(calls=1, accepted=1)
        assert engine.device_chain_stats()[1] - c0[1] == (1 if zero else 0)
        assert [rb.trace(w) for w in (3, 4, 5)] == want and rb.trace(8) == ZERO
    finally:
        engine.set_option("chain_test_zero", 0)  # (the fixture restores options to -1: this one's neutral value is 0)
        rb.close()


def test_with_the_recheck_of_rejections(bpp, packed, engine, opt, data):
    """verify_check = 1 and one bad proof: the fall-back's rejection is the one rechecked; outcome and recheck counters as without the
    joint check"""
    rb = _rb(packed, data, 7, _spoil(data[1], 4))
    try:
        opt("verify_check", 1)
        v0 = engine.verify_check_stats()
        off = packed.verify_groups(rb, BOUNDS)
        v1 = engine.verify_check_stats()
        opt("verify_joint", 1)
        s0 = engine.verify_joint_stats()
        assert packed.verify_groups(rb, BOUNDS) == off
        v2 = engine.verify_check_stats()
        assert {k: v2[k] - v1[k] for k in v1} == {k: v1[k] - v0[k] for k in v1}
        assert v1["rechecked_groups"] - v0["rechecked_groups"] == 1 and v1["confirmed"] - v0["confirmed"] == 1
        assert _delta(engine, s0) == _counts(calls=1, fallbacks=1)
    finally:
        rb.close()


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("bad", [None, 4])
def test_both_msm_plans(bpp, packed, engine, opt, data, split, bad):
    """msm_split forced off and on: both plans of the joint group (and of the fall-back) give the per-group outcome"""
    rb = _rb(packed, data, 7, None if bad is None else _spoil(data[1], bad))
    try:
        opt("msm_split", split)
        off = packed.verify_groups(rb, BOUNDS)
        opt("verify_joint", 1)
        s0 = engine.verify_joint_stats()
        assert packed.verify_groups(rb, BOUNDS) == off
        if bad is None:
            plan = engine.msm_last_plan()
            assert plan["G"] == 1 and plan["terms"] == (COLS + 7 * DYN) * (2 if split else 1), plan
            assert _delta(engine, s0) == _counts(calls=1, accepted=1) and rb.trace(8) == ZERO
        else:
            assert _delta(engine, s0) == _counts(calls=1, fallbacks=1) and rb.trace(8) != ZERO
    finally:
        rb.close()


def test_aggregated_proofs(bpp, engine, opt):
    """m = 2 at 8 bits (oracle-made proofs), five proofs as chunks of 2 + 2 + 1.  16 generator pairs per proof are no multiple of
    64, so this shape has ONE form of the generator columns, the per-proof rows, whatever "fused_columns" says: BPP_TRACE_PLAN's
    bit 0 is asserted clear with the option at 1.  Both forms: test_both_forms_of_the_generator_columns"""
    case = H.make_batch(bpp, engine, 8, [2] * 5, 1, seed=b"joint-m2")
    rb = bpp.ResidentBatch(case.transcripts(), case.statements_public, case.proofs)
    try:
        opt("fused_columns", 1)
        rb.verify(bpp.VerifyAction.VerifyOnly, chunk=2)
        want = [rb.trace(w) for w in (3, 4, 5, 7)]
        assert int(np.frombuffer(want[3], dtype=np.uint32)[0]) & 3 == 0
        opt("verify_joint", 1)
        s0 = engine.verify_joint_stats()
        rb.verify(bpp.VerifyAction.VerifyOnly, chunk=2)
        assert _delta(engine, s0) == _counts(calls=1, accepted=1)
        assert [rb.trace(w) for w in (3, 4, 5, 7)] == want and rb.trace(8) == ZERO
        plan = engine.msm_last_plan()
        assert plan["G"] == 1 and plan["terms"] == 2 * (2 * 16 + 2 + rb.shape()["total_dyn"])
    finally:
        rb.close()
        case.params.close()


@pytest.mark.parametrize("fused", [0, 1])
def test_both_forms_of_the_generator_columns(bpp, packed, engine, opt, data, fused):
    """eight 64-bit proofs as chunks of 4 + 4: 64 generator pairs per proof and every group on a workgroup boundary of k_scalars_lanes
    (four proofs, or a divisor of four), so the shape can take the column sums inside that kernel as well as the per-proof rows.
    BPP_TRACE_PLAN's bit 0 says which one ran: it follows the option, and the joint row is formed from either"""
    rb = _rb(packed, data, 8)
    try:
        opt("fused_columns", fused)
        rb.verify_only(chunk=4)
        want = [rb.trace(w) for w in (3, 4, 5, 7)]
        assert int(np.frombuffer(want[3], dtype=np.uint32)[0]) & 1 == fused
        opt("verify_joint", 1)
        s0 = engine.verify_joint_stats()
        rb.verify_only(chunk=4)
        assert _delta(engine, s0) == _counts(calls=1, accepted=1)
        assert [rb.trace(w) for w in (3, 4, 5, 7)] == want and rb.trace(8) == ZERO
    finally:
        rb.close()


def test_traces_after_passes_that_take_no_joint_check(bpp, packed, engine, opt, data):
    """trace(8) is the point of the last pass that TOOK the joint path, trace(6) is refused only while the last MSM of the batch was
    an accepted joint check: a recheck's passes 2 and 3 behind a fall-back leave trace(8) standing, and a pass with the option off
    brings trace(6) back without taking trace(8) away"""
    rb = _rb(packed, data, 7, _spoil(data[1], 4))
    good = _rb(packed, data, 7)
    try:
        opt("verify_joint", 1)
        opt("verify_check", 1)
        s0 = engine.verify_joint_stats()
        res = packed.verify_groups(rb, BOUNDS)
        assert [r["code"] != 0 for r in res] == [False, False, True, False]
        assert _delta(engine, s0)["fallbacks"] >= 1  # (pass 1; a third pass would be another joint pass)
        joint = rb.trace(8)  # pass 2 ran behind the joint pass: the point is still there
        assert joint != ZERO and len(rb.trace(6)) == 4 * 32
        opt("verify_check", 0)
        for value in (1, 0, 1):
            opt("verify_joint", value)
            assert all(r["code"] == 0 for r in packed.verify_groups(good, BOUNDS))
            assert good.trace(8) == ZERO  # (with the option off: the earlier pass's)
            if value:
                with pytest.raises(bpp.ProofError):
                    good.trace(6)
            else:
                assert good.trace(6) == ZERO * 4
    finally:
        good.close()
        rb.close()


def test_batcher_lanes_take_the_option(bpp, packed, engine, opt, data):
    """three threads with one 2-proof batch each, one of them invalid, pooled into one grouped call of three groups"""
    params, d = data
    bad = _spoil(d, 3)

    def inp(lo, proofs):
        sl = slice(lo, lo + 2)
        return packed.PackedInput(proofs[sl], d["commitments"][sl], d["min_values"][sl], d["min_present"][sl], None, LABEL)
    inputs = [inp(0, d["proofs"]), inp(2, bad), inp(4, d["proofs"])]
    want = []
    for x in inputs:
        try:
            packed.verify_batch(params, x, bpp.VerifyAction.VerifyOnly, 0)
            want.append((0, ""))
        except bpp.ProofError as e:
            want.append((int(e.kind), str(e)))
    assert [w[0] for w in want] == [0, int(bpp.ProofErrorKind.VerificationFailed), 0]
    opt("verify_joint", 1)  # before the batcher is made: its lanes copy the option
    # (one lane, and a leader that waits for company until all three calls are queued: the pooled call has three groups)
    bat = packed.Batcher(params, inputs[0], lanes=1, max_wait_us=20_000_000, max_calls=3)
    try:
        s0 = bat.verify_joint_stats()
        got = [None] * 3

        def caller(k):
            try:
                bat.verify(inputs[k])
                got[k] = (0, "")
            except bpp.ProofError as e:
                got[k] = (int(e.kind), str(e))
            except BaseException as e:  # noqa: BLE001
                got[k] = ("exception", repr(e))
        ths = [threading.Thread(target=caller, args=(k,)) for k in range(3)]
        for t in ths:
            t.start()
        for t in ths:
            t.join(timeout=120)
        assert not any(t.is_alive() for t in ths), "a caller is stuck in the batcher"
        assert got == want
        s1 = bat.verify_joint_stats()
        assert {k: s1[k] - s0[k] for k in STATS} == _counts(calls=1, fallbacks=1)
        lib_s = bpp._lib.VerifyJointStats()
        assert engine.lib.bpp_batcher_verify_joint_stats(bat.handle, ctypes.byref(lib_s)) == 0 and int(lib_s.calls) == s1["calls"]
    finally:
        bat.close()


def test_batcher_lane_made_by_the_batcher_takes_the_option(bpp, packed, engine, opt, data):
    """two lanes: the first is the caller's context, the second a context the batcher makes -- and it must take "verify_joint" from
    the caller's.  Two callers, pools of two: whichever caller enters first leads the first lane and waits there for company; the
    other finds the second lane free, needs no company any more (two requests are queued) and takes both before it lets go of the
    pool's lock.  So the call of two groups runs on the made lane whatever the threads' order, and the made lane's counters -- the
    batcher's sum less the caller's context's -- are the ones that move"""
    params, d = data
    bad = _spoil(d, 3)

    def inp(lo, proofs):
        sl = slice(lo, lo + 2)
        return packed.PackedInput(proofs[sl], d["commitments"][sl], d["min_values"][sl], d["min_present"][sl], None, LABEL)
    rounds = [[inp(0, d["proofs"]), inp(4, d["proofs"])], [inp(0, d["proofs"]), inp(2, bad)]]
    try:
        packed.verify_batch(params, rounds[1][1], bpp.VerifyAction.VerifyOnly, 0)
        failed = None
    except bpp.ProofError as e:  # what this caller gets from a call of its own
        failed = (int(e.kind), str(e))
    assert failed and failed[0] == int(bpp.ProofErrorKind.VerificationFailed)
    opt("verify_joint", 1)  # before the batcher is made: its lanes copy the option
    bat = packed.Batcher(params, rounds[0][0], lanes=2, max_wait_us=20_000_000, max_calls=2)
    try:
        for inputs, want, counted in ((rounds[0], [(0, ""), (0, "")], _counts(calls=1, accepted=1)),
                                      (rounds[1], [(0, ""), failed], _counts(calls=1, fallbacks=1))):
            b0, e0 = bat.verify_joint_stats(), engine.verify_joint_stats()
            got = [None] * 2

            def caller(k):
                try:
                    bat.verify(inputs[k])
                    got[k] = (0, "")
                except bpp.ProofError as e:
                    got[k] = (int(e.kind), str(e))
                except BaseException as e:  # noqa: BLE001
                    got[k] = ("exception", repr(e))
            ths = [threading.Thread(target=caller, args=(k,)) for k in range(2)]
            for t in ths:
                t.start()
            for t in ths:
                t.join(timeout=120)
            assert not any(t.is_alive() for t in ths), "a caller is stuck in the batcher"
            assert got == want
            b1 = bat.verify_joint_stats()
            assert {k: b1[k] - b0[k] for k in STATS} == counted
            assert _delta(engine, e0) == _counts(), "the pooled call ran on the caller's own context"
        assert bat.stats()["pooled_calls"] == 4
    finally:
        bat.close()


def test_transcript_states_are_unchanged(bpp, packed, engine, opt, data):
    rb = _rb(packed, data, 12)
    try:
        _, off = rb.verify(bpp.VerifyAction.VerifyOnly, chunk=5, states=True)
        opt("verify_joint", 1)
        s0 = engine.verify_joint_stats()
        _, on = rb.verify(bpp.VerifyAction.VerifyOnly, chunk=5, states=True)
        assert on == off and len(on) == 12 and all(len(r) == 203 for r in on)
        assert _delta(engine, s0) == _counts(calls=1, accepted=1)
    finally:
        rb.close()


def test_rule_bound_on_the_joint_group(bpp, packed, engine, opt):
    """the joint form is taken while the joint group has at most 14 000 terms (engine.hip: BPP_JOINT_MAX_TERMS; above, it measured
    slower than the per-group MSMs): 866 proofs give 130 + 16 x 866 = 13 986 terms, 868 give 14 018.  "verify_joint" = 2 takes it
    whatever the size -- here through the one-workgroup prelude at 11 bits, with the same verdicts"""
    import bench
    params = bpp.RangeParameters.init(64, 1, bpp.create_pedersen_gens_with_extension_degree(1), engine=engine)
    try:
        d = bench.make_inputs(np, packed, params, 868, seed=20261021)
        for n, value, want in ((866, 1, _counts(calls=1, accepted=1)), (868, 1, _counts()), (868, 2, _counts(calls=1, accepted=1))):
            rb = packed.ResidentBatch(params, d["proofs"][:n], d["commitments"][:n], d["min_values"][:n], d["min_present"][:n], None, LABEL)
            try:
                opt("verify_joint", value)
                s0 = engine.verify_joint_stats()
                rb.verify_only(chunk=n // 2)
                assert _delta(engine, s0) == want, (n, value)
                plan = engine.msm_last_plan()
                assert (plan["G"], plan["terms"]) == ((1, (COLS + DYN * n) * (2 if n == 866 else 1)) if want["calls"] else (2, 2 * COLS + DYN * n)), plan
                if n == 866:
                    # only the joint plan is a half-scalar one here (13 986 terms against the per-group plan's 14 116): the option
                    # off and on again over the same layout, and the joint check still has its points' upper halves
                    for value2, want2 in ((0, _counts()), (1, _counts(calls=1, accepted=1))):
                        opt("verify_joint", value2)
                        s0 = engine.verify_joint_stats()
                        rb.verify_only(chunk=n // 2)
                        assert _delta(engine, s0) == want2, value2
                        assert engine.msm_last_plan()["terms"] == (2 * (COLS + DYN * n) if value2 else 2 * COLS + DYN * n)
                    assert rb.trace(8) == ZERO
            finally:
                rb.close()
    finally:
        params.close()
