"""GPU tests: the device's Merlin sponges at every starting position of the 166-byte block.

Whether the word-wise absorb of csrc/lstrobe.h, the lane-strided chunks of csrc/wstrobe.h and the byte loop of csrc/merlin.h take
their boundary branches depends only on where in the block an operation starts, and before a proof's first challenge that is the
caller's doing: the transcript label and whatever context went in.  tests/transcript_sweep.py holds one proof per position (166
label lengths, two shapes; tests/test_transcript_sweep.py asserts that they reach every alignment); here every kernel form that
runs a sponge is held to the oracle over them, byte for byte:

  verifier PASS 1   k_transcripts<false|true> (one lane per transcript), k_transcripts_wave<false|true> (one wavefront), transcripts
                    given as labels and as 203-byte states: challenges, transcript-RNG bytes, weights, scalars, masks, and the
                    advanced states of bpp_verify_batch_states / bpp_verify_resident_states
  prover            kp_init, kp_lane + kp_wave ("prove_fused" = 0), kp_round<1|2|4> ("prove_waves"), labels and states in, and the
                    advanced states of bpp_prove_batch_mixed_states

Expected values come from the C oracle (proofs, traces, masks) and from oracle.pyref (states).  They are made once per process.
Every comparison is per item: a failure names the label length, the starting position, the kernel form and the first trace that
differs."""
import time
import types

import pytest

from oracle.pyref import merlin as M
from oracle.pyref import protocol as O
from tests import transcript_sweep as TS
from tests.helpers import replay_verifier_state

pytestmark = pytest.mark.gpu

SHARED = {}
PROVER_FORMS = {"three-launches": {"prove_fused": 0}, "fused-1": {"prove_fused": 1, "prove_waves": 1},
                "fused-2": {"prove_fused": 1, "prove_waves": 2}, "fused-4": {"prove_fused": 1, "prove_waves": 4}}


def case(bpp, engine, shape):
    return TS.attach(TS.sweep(shape), bpp, engine)


def verifier_states(c):
    """what the oracle's verify() leaves in each item's transcript: its PASS 1 replayed, hashes only"""
    key = ("verifier-states", c.name)
    if key not in SHARED:
        pc = O.PedersenGens(c.t)
        SHARED[key] = [replay_verifier_state(M.Transcript(label), c.n, c.t, pc, comm, mins, raw)
                       for label, comm, mins, raw in zip(c.labels, c.commitments, c.mins, c.raw)]
    return SHARED[key]


PROVER_EDGE_POSITIONS = (0, 1, 2, 163, 164, 165)


def prover_slots(c):
    """the items whose prover state the Python oracle's prover is asked for: every third label length, and the six lengths that
    hand the sponge over at the two ends of the block"""
    return [k for k in range(len(c.items)) if c.lengths[k] % 3 == 0 or c.positions[k] in PROVER_EDGE_POSITIONS]


def prover_states(c):
    """{call slot: what the Python oracle's prover leaves in that item's transcript} (its proofs are the C oracle's, byte for byte)"""
    key = ("prover-states", c.name)
    if key not in SHARED:
        o_params = O.RangeParameters(c.n, c.m, O.PedersenGens(c.t))
        out = {}
        for k in prover_slots(c):
            st, w = TS.oracle_statement(c, k, o_params)
            tr = M.Transcript(c.labels[k])
            assert O.prove_with_rng(tr, st, w, M.ByteStreamRng(c.ext[k])).to_bytes() == c.raw[k], c.describe(k)
            out[k] = tr.strobe.to_bytes()
        SHARED[key] = out
    return SHARED[key]


def replayed_prover_states(c):
    """the prover's transcript of every item by hashing alone: the prover's own transcript (not the clones its nonces come from)
    absorbs what the verifier's does, up to the last challenge"""
    key = ("replayed-prover-states", c.name)
    if key not in SHARED:
        pc = O.PedersenGens(c.t)
        out = []
        for label, comm, mins, raw in zip(c.labels, c.commitments, c.mins, c.raw):
            proof = O.RangeProof.from_bytes(raw)
            tr = M.Transcript(label)
            st = types.SimpleNamespace(commitments_compressed=comm, minimum_value_promises=mins)
            rpt = O.RangeProofTranscript(tr, pc.h_base_compressed, pc.g_base_compressed_vec, c.n, c.t, c.m, st, None, M.NullRng())
            rpt.challenges_y_z(proof.a)
            for l, r in zip(proof.li, proof.ri):
                rpt.challenge_round_e(l, r)
            rpt.challenge_final_e(proof.a1, proof.b)
            out.append(tr.strobe.to_bytes())
        SHARED[key] = out
    return SHARED[key]


def resident_pass(bpp, c, transcripts, proofs, form, states=False):
    """a resident batch as ONE reference batch: traces 1 .. 5 equal the oracle's, the batch is accepted, the final point is the
    identity, the masks are the oracle's.  A wrong sponge makes the batch fail in its sum: the traces are read all the same (they
    stay in place after a rejection), so that the failure names the item and the trace, not just the verdict.  -> the states"""
    rb = bpp.ResidentBatch(transcripts, c.statements, proofs)
    verdict = out = None
    try:
        try:
            out = rb.verify(bpp.VerifyAction(c.action), chunk=0, states=states)
        except bpp.ProofError as e:
            verdict = e
        got = {name: rb.trace(what) for name, what in TS.TRACE_IDS}
        final = rb.trace(6)
    finally:
        rb.close()
    diff = TS.first_trace_difference(c, got)
    assert diff is None, "%s: %s%s" % (form, diff, "" if verdict is None else " [and the batch was rejected: %s]" % verdict)
    assert verdict is None, "%s: every trace equals the oracle's, yet: %s" % (form, verdict)
    assert final == bytes(32), form
    masks, rows = out if states else (out, None)
    for k, (m, w) in enumerate(zip(masks, c.masks)):
        assert (m.blindings() if m is not None else None) == w, "%s: %s: the recovered mask differs" % (form, c.describe(k))
    return rows


# ---------------------------------------------------------------------------------------------------------- verifier PASS 1
@pytest.mark.parametrize("how", ["labels", "states"])
@pytest.mark.parametrize("wave", [0, 1], ids=["k_transcripts", "k_transcripts_wave"])
@pytest.mark.parametrize("shape", ["A", "B"])
def test_pass1_equals_the_oracle_at_every_position(bpp, engine, opt, shape, wave, how):
    c = case(bpp, engine, shape)
    opt("transcripts_wave", wave)
    resident_pass(bpp, c, TS.transcripts(bpp, c, how), c.proofs, "transcripts_wave = %d, transcripts as %s" % (wave, how))


@pytest.mark.parametrize("wave", [0, 1], ids=["k_transcripts", "k_transcripts_wave"])
@pytest.mark.parametrize("shape", ["A", "B"])
def test_verifier_states_equal_the_oracle_at_every_position(bpp, engine, opt, shape, wave):
    """the state-returning instantiations: bpp_verify_resident_states and bpp_verify_batch_states, labels in and states in"""
    c = case(bpp, engine, shape)
    want = verifier_states(c)
    opt("transcripts_wave", wave)
    for how in ("labels", "states"):
        form = "transcripts_wave = %d, bpp_verify_resident_states, transcripts as %s" % (wave, how)
        got = resident_pass(bpp, c, TS.transcripts(bpp, c, how), c.proofs, form, states=True)
        diff = TS.first_state_difference(c, got, want, "the advanced verifier state")
        assert diff is None, "%s: %s" % (form, diff)
        form = form.replace("verify_resident", "verify_batch")
        trs = TS.transcripts(bpp, c, how)
        try:
            masks = bpp.RangeProof.verify_batch(trs, c.statements, c.proofs, bpp.VerifyAction(c.action), chunk=0, advance=True)
        except bpp.ProofError as e:  # (the resident form of the same kernel passed just above)
            raise AssertionError("%s: rejected: %s" % (form, e))
        diff = TS.first_state_difference(c, [tr.state for tr in trs], want, "the advanced verifier state")
        assert diff is None, "%s: %s" % (form, diff)
        assert [m.blindings() if m is not None else None for m in masks] == c.masks, form


# ------------------------------------------------------------------------------------------------------------------ prover
def prove(bpp, c, how, form, advance=False):
    """166 proofs in one bpp_prove_batch_mixed call -> (proof bytes, the transcript objects); every one must be the oracle's"""
    trs = TS.transcripts(bpp, c, how)
    made = bpp.RangeProof.prove_batch_mixed(trs, c.statements, c.witnesses, c.ext, advance=advance)
    for k, p in enumerate(made):
        assert not isinstance(p, Exception), "%s: %s: %r" % (form, c.describe(k), p)
    raw = [p.to_bytes() for p in made]
    diff = TS.first_state_difference(c, raw, c.raw, "the proof")
    assert diff is None, "%s: %s" % (form, diff)
    return made, trs


@pytest.mark.parametrize("form", list(PROVER_FORMS))
@pytest.mark.parametrize("shape", ["A", "B"])
def test_proofs_equal_the_oracle_at_every_position(bpp, engine, opt, shape, form):
    """shape B draws every nonce from a TranscriptRng cloned and re-keyed at the swept position; shape A has a seed nonce"""
    c = case(bpp, engine, shape)
    for name, value in PROVER_FORMS[form].items():
        opt(name, value)
    prove(bpp, c, "labels", "prover form %s, transcripts as labels" % form)


@pytest.mark.parametrize("shape", ["A", "B"])
def test_proofs_from_states_equal_the_oracle_at_every_position(bpp, engine, shape):
    c = case(bpp, engine, shape)
    prove(bpp, c, "states", "the engine's own prover form, transcripts as states")


def test_prover_states_equal_the_oracle_at_every_position(bpp, engine):
    """bpp_prove_batch_mixed_states over shape A, labels in and states in.  Only the Python oracle's prover returns a transcript,
    and it takes 0.21 s per proof of shape A on the CPU, 35 s for 166: it is asked for every third label length plus the six lengths
    that start at positions 0, 1, 2, 163, 164, 165 (60 proofs, 10 s; the time is printed).  All 166 states are compared with a
    hash-only replay of the prover's transcript, which in turn must equal the oracle prover's on those 60."""
    c = case(bpp, engine, "A")
    t0 = time.perf_counter()
    want = prover_states(c)
    print("oracle prover, %d proofs of shape A: %.1f s" % (len(want), time.perf_counter() - t0))
    assert {c.positions[k] for k in want} >= set(PROVER_EDGE_POSITIONS) and len(want) >= 56 + 4
    replayed = replayed_prover_states(c)
    for k, state in want.items():
        assert replayed[k] == state, c.describe(k)
    for how in ("labels", "states"):
        form = "bpp_prove_batch_mixed_states, transcripts as %s" % how
        _, trs = prove(bpp, c, how, form, advance=True)
        for k, state in want.items():
            assert trs[k].state == state, "%s: %s: the advanced prover state differs from the oracle prover's" % (form, c.describe(k))
        diff = TS.first_state_difference(c, [tr.state for tr in trs], replayed, "the advanced prover state")
        assert diff is None, "%s: %s" % (form, diff)


@pytest.mark.parametrize("shape", ["A", "B"])
def test_round_trip_at_every_position(bpp, engine, shape):
    """the engine's proofs through the engine's verifier, both in their own default forms: accepted, traces as the oracle's, masks
    recovered"""
    c = case(bpp, engine, shape)
    made, _ = prove(bpp, c, "labels", "round trip, prover")
    resident_pass(bpp, c, TS.transcripts(bpp, c, "labels"), made, "round trip, verifier")
