"""GPU tests: the transcripts come back advanced from device-side verify and prove (bpp_verify_batch_states,
bpp_verify_batch_packed_states, bpp_verify_resident_states, bpp_prove_batch_mixed_states, bpp_prove_openings_states and the
advance=True / states=True forms of the Python mirrors).

The oracle is oracle.pyref, whose Transcript objects are advanced in place by verify() and prove_with_rng();
`t.strobe.to_bytes()` is the 203-byte comparison.  The inputs carry context: a message appended to the transcript before the
call.  Two sub-checks cannot, and say so where they stand: "label in against state in" needs a transcript that a label alone
describes, and the 70 proofs of the lane-form test come from the C oracle, which proves under a label only; the same 70-proof
shape is therefore run a second time with context, over proofs the engine's own prover made from context-carrying transcripts.

Oracle work is done once per module (SHARED) and never modified."""
import ctypes

import numpy as np
import pytest

from oracle import cport
from oracle.pyref import merlin as M
from oracle.pyref import protocol as O
from tests.helpers import Prng, replay_verifier_state, sb

pytestmark = pytest.mark.gpu

N = 64
LABEL, CTX_LABEL, CTX = b"outer protocol v1", b"block-context", bytes(range(40, 97))
PREFILL = 0xA5
SHARED = {}


def o_transcript(context=True):
    t = M.Transcript(LABEL)
    if context:
        t.append_message(CTX_LABEL, CTX)
    return t


def p_transcripts(bpp, n, how="ops"):
    """the product's transcripts in the oracle's starting state: by the mirror's own operations, or from the oracle's bytes"""
    out = []
    for _ in range(n):
        if how == "ops":
            t = bpp.Transcript.new(LABEL)
            t.append_message(CTX_LABEL, CTX)
        else:
            t = bpp.Transcript.from_state(o_transcript().strobe.to_bytes())
        out.append(t)
    return out


class Case:
    pass


def oracle_case(t, aggregation, seed, prove=True):
    """statements and witnesses for `aggregation` (seed nonce on the m = 1 items, a promise on every opening); with `prove` the
    oracle's prover runs on context-carrying transcripts: c.raw (proof bytes), c.prover_states (the transcripts it leaves)"""
    key = (t, tuple(aggregation), seed, prove)
    if key in SHARED:
        return SHARED[key]
    rng = Prng(seed)
    c = Case()
    c.t, c.aggregation = t, list(aggregation)
    c.o_params = O.RangeParameters(N, max(aggregation), O.PedersenGens(t))
    c.o_statements, c.o_witnesses, c.ext, c.raw, c.prover_states = [], [], [], [], []
    for m in aggregation:
        openings, comms, mins = [], [], []
        for _ in range(m):
            v = rng.next_u64() % (1 << (N - 1))
            blind = [O.random_not_zero(rng) for _ in range(t)]
            openings.append(O.CommitmentOpening(v, blind))
            comms.append(c.o_params.pc_gens.commit(v, blind))
            mins.append(v // 3)
        c.o_statements.append(O.RangeStatement(c.o_params, comms, mins, O.random_not_zero(rng) if m == 1 else None))
        c.o_witnesses.append(O.RangeWitness(openings))
        c.ext.append(rng.fill_bytes(32 * ((N * m).bit_length() - 1 + 3)))
    if prove:
        for st, w, ext in zip(c.o_statements, c.o_witnesses, c.ext):
            tr = o_transcript()
            c.raw.append(O.prove_with_rng(tr, st, w, M.ByteStreamRng(ext)).to_bytes())
            c.prover_states.append(tr.strobe.to_bytes())
    SHARED[key] = c
    return c


def oracle_verifier_states(c, raw):
    """the oracle's verify() (RecoverAndVerify) over the case's statements and `raw`: it raises unless the batch is valid, and
    leaves every transcript advanced -> (states, masks)"""
    trs = [o_transcript() for _ in raw]
    masks = O.verify(trs, c.o_statements, [O.RangeProof.from_bytes(r) for r in raw], 1)
    return [tr.strobe.to_bytes() for tr in trs], [[sb(x) for x in m] if m is not None else None for m in masks]


def attach(c, bpp, engine):
    if hasattr(c, "params"):
        return c
    c.params = bpp.RangeParameters.init(N, max(c.aggregation), bpp.create_pedersen_gens_with_extension_degree(c.t), engine=engine)
    c.statements = [bpp.RangeStatement.init(c.params, list(s.commitments_compressed), s.minimum_value_promises,
                                            sb(s.seed_nonce) if s.seed_nonce is not None else None) for s in c.o_statements]
    c.witnesses = [bpp.RangeWitness.init([bpp.CommitmentOpening.new(o.v, [sb(r) for r in o.r]) for o in w.openings]) for w in c.o_witnesses]
    return c


def verify_case(bpp, engine, t):
    """five proofs with m = 1, 2, 4, 1, 2 over context-carrying transcripts, and the oracle's verifier states and masks for them.
    t = 1: the oracle's own proofs; t = 2: proofs the engine's prover made, which the oracle's verify() then accepts."""
    key = ("verify", t)
    if key in SHARED:
        return SHARED[key]
    c = attach(oracle_case(t, [1, 2, 4, 1, 2], b"states-%d" % t, prove=(t == 1)), bpp, engine)
    if t != 1:
        made = bpp.RangeProof.prove_batch_mixed(p_transcripts(bpp, 5), c.statements, c.witnesses, c.ext)
        c.raw = [p.to_bytes() for p in made]
    c.proofs = [bpp.RangeProof.from_bytes(r) for r in c.raw]
    c.verifier_states, c.masks = oracle_verifier_states(c, c.raw)
    SHARED[key] = c
    return c


def masks_of(res):
    return [m.blindings() if m is not None else None for m in res]


def states_call(bpp, c, transcripts, action, chunk):
    res = bpp.RangeProof.verify_batch(transcripts, c.statements, c.proofs, action, chunk=chunk, advance=True)
    return [tr.state for tr in transcripts], masks_of(res)


# ------------------------------------------------------------------------------------------------------------- 1. item form
@pytest.mark.parametrize("t", [1, 2])
def test_item_form_states_equal_the_oracle_in_both_kernels(bpp, engine, opt, t):
    c = verify_case(bpp, engine, t)
    A = bpp.VerifyAction
    plain = masks_of(bpp.RangeProof.verify_batch(p_transcripts(bpp, 5), c.statements, c.proofs, A.RecoverAndVerify, chunk=0))
    assert plain == c.masks
    for wave in (1, 0):
        opt("transcripts_wave", wave)
        got, masks = states_call(bpp, c, p_transcripts(bpp, 5), A.RecoverAndVerify, 0)
        assert got == c.verifier_states, "transcripts_wave = %d" % wave
        assert masks == plain  # masks and verdict as without the buffer


@pytest.mark.parametrize("t", [1, 2])
def test_item_form_states_do_not_depend_on_action_chunk_or_kernel(bpp, engine, opt, t):
    c = verify_case(bpp, engine, t)
    A = bpp.VerifyAction
    for wave in (1, 0):
        opt("transcripts_wave", wave)
        for action in (A.VerifyOnly, A.RecoverAndVerify, A.RecoverOnly):
            for chunk in (0, 2):
                for how in ("ops", "bytes"):
                    got, masks = states_call(bpp, c, p_transcripts(bpp, 5, how), action, chunk)
                    assert got == c.verifier_states, (wave, action, chunk, how)
                    want = masks_of(bpp.RangeProof.verify_batch(p_transcripts(bpp, 5), c.statements, c.proofs, action, chunk=chunk))
                    assert masks == want == (c.masks if action != A.VerifyOnly else [None] * 5)


def label_case(bpp, engine, t, aggregation, seed):
    """proofs from the C oracle, which proves under a label: the transcripts carry NO context here (see the module's docstring).
    The expected states are the oracle's PASS 1 replayed on Transcript::new(LABEL)."""
    key = ("label", t, tuple(aggregation), seed)
    if key in SHARED:
        return SHARED[key]
    c = attach(oracle_case(t, aggregation, seed, prove=False), bpp, engine)
    cp = cport.Params(N, max(aggregation), t)
    c.raw = []
    for st, w, ext in zip(c.o_statements, c.o_witnesses, c.ext):
        raw, comm = cp.prove(LABEL, [o.v for o in w.openings], [[sb(r) for r in o.r] for o in w.openings], st.minimum_value_promises,
                             sb(st.seed_nonce) if st.seed_nonce is not None else None, ext)
        assert comm == list(st.commitments_compressed)
        c.raw.append(raw)
    cp.close()
    c.proofs = [bpp.RangeProof.from_bytes(r) for r in c.raw]
    pc = c.o_params.pc_gens
    c.verifier_states = [replay_verifier_state(o_transcript(False), N, t, pc, st.commitments_compressed, st.minimum_value_promises, raw)
                         for st, raw in zip(c.o_statements, c.raw)]
    SHARED[key] = c
    return c


@pytest.mark.parametrize("t", [1, 2])
def test_label_in_and_state_in_give_the_same_states(bpp, engine, opt, t):
    c = label_case(bpp, engine, t, [1, 2, 4, 1, 2], b"label-in-%d" % t)
    A = bpp.VerifyAction
    for wave in (1, 0):
        opt("transcripts_wave", wave)
        by_label, m1 = states_call(bpp, c, [bpp.Transcript.new(LABEL) for _ in range(5)], A.RecoverAndVerify, 0)
        by_state, m2 = states_call(bpp, c, [bpp.Transcript.from_state(o_transcript(False).strobe.to_bytes()) for _ in range(5)],
                                   A.RecoverAndVerify, 0)
        assert by_label == by_state == c.verifier_states, wave
        assert m1 == m2


# ------------------------------------------------------------------------------------- 2. lane form across a wavefront boundary
def packed_input(bpp, c, state=None):
    packed = __import__("importlib").import_module("bulletproofs-plus_amd.packed")
    n = len(c.raw)
    proofs = np.frombuffer(b"".join(c.raw), dtype=np.uint8).reshape(n, -1)
    comm = np.frombuffer(b"".join(b"".join(s.commitments_compressed) for s in c.o_statements), dtype=np.uint8).reshape(n, 1, 32)
    mins = np.array([[s.minimum_value_promises[0]] for s in c.o_statements], dtype=np.uint64)
    pres = np.ones((n, 1), dtype=np.uint8)
    seeds = np.frombuffer(b"".join(sb(s.seed_nonce) for s in c.o_statements), dtype=np.uint8).reshape(n, 32)
    return packed, packed.PackedInput(proofs, comm, mins, pres, seeds, LABEL, state=state)


def three_forms(bpp, c, make_transcripts, state):
    """the item form, the packed form and a resident batch over the same 70 proofs -> three lists of 203-byte states"""
    A = bpp.VerifyAction
    item, _ = states_call(bpp, c, make_transcripts(), A.VerifyOnly, 0)
    packed, inp = packed_input(bpp, c, state)
    _, _, st = packed.verify_batch(c.params, inp, A.VerifyOnly, chunk=0, states=True)
    assert st.shape == (len(c.raw), 203) and st.dtype == np.uint8
    rb = bpp.ResidentBatch(make_transcripts(), c.statements, c.proofs)
    rb.verify_only(chunk=0)  # (without the buffer first: the batch's later call with it must not depend on that)
    masks, res = rb.verify(A.RecoverAndVerify, chunk=0, states=True)
    again = rb.verify(A.RecoverAndVerify, chunk=0)  # and without it again: the masks alone, as ever
    rb.close()
    assert masks == again
    return item, [bytes(r) for r in st], res


def test_lane_form_two_wavefronts_the_second_with_six_live_lanes(bpp, engine, opt):
    c = label_case(bpp, engine, 1, [1] * 70, b"seventy")
    opt("transcripts_wave", 0)
    item, packed, resident = three_forms(bpp, c, lambda: [bpp.Transcript.new(LABEL) for _ in range(70)], None)
    assert item == c.verifier_states
    assert packed == item and resident == item


def test_lane_form_seventy_proofs_with_context(bpp, engine, opt):
    """the same shape with context: 70 proofs the engine's prover makes from context-carrying transcripts (two sub-batches of the
    prover: 64 + 6), its states held to the verifier's by the composition rule, the verifier's to the oracle's replay"""
    c = attach(oracle_case(1, [1] * 70, b"seventy-ctx", prove=False), bpp, engine)
    trs = p_transcripts(bpp, 70)
    made = bpp.RangeProof.prove_batch_mixed(trs, c.statements, c.witnesses, c.ext, advance=True)
    c.raw = [p.to_bytes() for p in made]
    c.proofs = made
    pc = c.o_params.pc_gens
    want = [replay_verifier_state(o_transcript(), N, 1, pc, st.commitments_compressed, st.minimum_value_promises, raw)
            for st, raw in zip(c.o_statements, c.raw)]
    for tr, raw in zip(trs, c.raw):  # prover's state + r1, s1, d1 = verifier's state
        tr.append_message(b"r1", raw[1 + 32 + 96:1 + 32 + 128])
        tr.append_message(b"s1", raw[1 + 32 + 128:1 + 32 + 160])
        tr.append_message(b"d1", raw[1:33])
    assert [tr.state for tr in trs] == want
    state0 = o_transcript().strobe.to_bytes()
    opt("transcripts_wave", 0)
    item, packed, resident = three_forms(bpp, c, lambda: [bpp.Transcript.from_state(state0) for _ in range(70)], state0)
    assert item == want and packed == want and resident == want
    opt("transcripts_wave", 1)
    assert states_call(bpp, c, p_transcripts(bpp, 70), bpp.VerifyAction.VerifyOnly, 0)[0] == want


# ------------------------------------------------------------------------------------------------------------------ 3. failures
def raw_verify_states(bpp, c, proofs, transcripts, action=0, chunk=0):
    """bpp_verify_batch_states with a prefilled state buffer -> (rc, message, the buffer)"""
    eng = c.params.engine
    items, keep = bpp.RangeProof._items(transcripts, c.statements, proofs)
    n = len(proofs)
    masks = (ctypes.c_uint8 * (n * c.t * 32))()
    present = (ctypes.c_uint8 * n)()
    buf = (ctypes.c_uint8 * (203 * n))(*([PREFILL] * (203 * n)))
    err = ctypes.create_string_buffer(256)
    rc = eng.lib.bpp_verify_batch_states(eng.ctx, c.params.handle, items, n, action, chunk, masks, present, buf, err, 256)
    return rc, err.value.decode(errors="replace"), bytes(buf)


@pytest.mark.parametrize("wave", [1, 0])
@pytest.mark.parametrize("kind", ["r1-bit", "zero-A"])
def test_a_failed_verification_writes_nothing(bpp, engine, opt, kind, wave):
    c = verify_case(bpp, engine, 1)
    opt("transcripts_wave", wave)
    bad = bytearray(c.raw[2])
    if kind == "r1-bit":
        bad[1 + 32 + 96] ^= 1  # r1: the final multiscalar check rejects
    else:
        bad[1 + 32:1 + 64] = bytes(32)  # A = identity: a PASS-1 finding
    proofs = c.proofs[:2] + [bpp.RangeProof.from_bytes(bytes(bad))] + c.proofs[3:]
    rc, msg, buf = raw_verify_states(bpp, c, proofs, p_transcripts(bpp, 5))
    with pytest.raises(bpp.ProofError) as usual:
        bpp.RangeProof.verify_batch(p_transcripts(bpp, 5), c.statements, proofs, bpp.VerifyAction.VerifyOnly, chunk=0)
    assert rc == int(usual.value.kind) == 1 and msg == usual.value.msg
    assert buf == bytes([PREFILL]) * (203 * 5)
    trs = p_transcripts(bpp, 5)
    before = [(tr.label, tr.state) for tr in trs]
    with pytest.raises(bpp.ProofError):
        bpp.RangeProof.verify_batch(trs, c.statements, proofs, bpp.VerifyAction.VerifyOnly, chunk=0, advance=True)
    assert [(tr.label, tr.state) for tr in trs] == before
    # and the good batch through the same buffer: every row written
    rc, msg, buf = raw_verify_states(bpp, c, c.proofs, p_transcripts(bpp, 5))
    assert rc == 0 and [buf[203 * i:203 * i + 203] for i in range(5)] == c.verifier_states


def test_one_transcript_object_for_several_items_is_refused(bpp, engine):
    c = verify_case(bpp, engine, 1)
    one = p_transcripts(bpp, 1)[0]
    with pytest.raises(bpp.ProofError) as e:
        bpp.RangeProof.verify_batch([one] * 5, c.statements, c.proofs, bpp.VerifyAction.VerifyOnly, chunk=0, advance=True)
    assert e.value.kind == bpp.ProofErrorKind.InvalidArgument
    bpp.RangeProof.verify_batch([one] * 5, c.statements, c.proofs, bpp.VerifyAction.VerifyOnly, chunk=0)  # fine without advance


# -------------------------------------------------------------------------------------------------------------------- 4. prover
def prove_case(bpp, engine, t):
    return attach(oracle_case(t, [1, 2, 4, 1, 2] if t == 1 else [1, 2, 4], b"states-%d" % t), bpp, engine)


def raw_prove_states(bpp, c, statements):
    """bpp_prove_batch_mixed_states with a prefilled state buffer -> (rc, codes, proof bytes per item, the buffer's rows)"""
    n = len(statements)
    params, items, cnt, keep = bpp.RangeProof._prove_marshal(p_transcripts(bpp, n), statements, c.witnesses, c.ext)
    eng = params.engine
    stride = 1 + 32 * (6 + 5 + 2 * 12)
    out = (ctypes.c_uint8 * (stride * n))()
    lens = (ctypes.c_size_t * n)()
    status = (ctypes.c_int * n)()
    buf = (ctypes.c_uint8 * (203 * n))(*([PREFILL] * (203 * n)))
    err = ctypes.create_string_buffer(256)
    rc = eng.lib.bpp_prove_batch_mixed_states(eng.ctx, params.handle, items, n, out, stride, lens, status, buf, err, 256)
    raw = bytes(out)
    return rc, list(status), [raw[i * stride:i * stride + lens[i]] for i in range(n)], [bytes(buf)[203 * i:203 * i + 203] for i in range(n)]


@pytest.mark.parametrize("t", [1, 3])
def test_prover_states_equal_the_oracle(bpp, engine, opt, t):
    c = prove_case(bpp, engine, t)
    n = len(c.aggregation)
    plain = bpp.RangeProof.prove_batch_mixed(p_transcripts(bpp, n), c.statements, c.witnesses, c.ext)
    assert [p.to_bytes() for p in plain] == c.raw
    trs = p_transcripts(bpp, n)
    got = bpp.RangeProof.prove_batch_mixed(trs, c.statements, c.witnesses, c.ext, advance=True)
    assert [p.to_bytes() for p in got] == c.raw  # byte-equal to the call without states
    assert [tr.state for tr in trs] == c.prover_states
    # the openings form: the commitments made by the engine, the same states
    trs = p_transcripts(bpp, n, "bytes")
    sts, prs = bpp.RangeProof.prove_openings(trs, c.witnesses, [s.minimum_value_promises for s in c.o_statements],
                                             [s.seed_nonce for s in c.statements], c.ext, c.params, advance=True)
    assert [p.to_bytes() for p in prs] == c.raw
    assert [s.commitments_compressed for s in sts] == [s.commitments_compressed for s in c.statements]
    assert [tr.state for tr in trs] == c.prover_states
    # under the self-check: the same proofs, the same states
    opt("prove_check", 1)
    trs = p_transcripts(bpp, n)
    got = bpp.RangeProof.prove_batch_mixed(trs, c.statements, c.witnesses, c.ext, advance=True)
    assert [p.to_bytes() for p in got] == c.raw and [tr.state for tr in trs] == c.prover_states


@pytest.mark.parametrize("t", [1, 3])
def test_a_failed_prove_item_keeps_its_row(bpp, engine, t):
    c = prove_case(bpp, engine, t)
    n = len(c.aggregation)
    wrong = list(c.statements)
    s = c.statements[1]  # the m = 2 item: its two commitments swapped do not open to its witness
    wrong[1] = bpp.RangeStatement.init(c.params, s.commitments_compressed[::-1], s.minimum_value_promises, None)
    rc, codes, proofs, rows = raw_prove_states(bpp, c, wrong)
    assert rc == 2 and codes == [0, 2] + [0] * (n - 2)
    assert rows[1] == bytes([PREFILL]) * 203 and proofs[1] == bytes(len(proofs[1]))
    for i in range(n):
        if i != 1:
            assert rows[i] == c.prover_states[i] and proofs[i] == c.raw[i], i
    # the advancing mirror: the failed item's transcript object is untouched, the others are advanced
    trs = p_transcripts(bpp, n)
    before = (trs[1].label, trs[1].state)
    res = bpp.RangeProof.prove_batch_mixed(trs, wrong, c.witnesses, c.ext, advance=True)
    assert isinstance(res[1], bpp.ProofError) and (trs[1].label, trs[1].state) == before
    assert [tr.state for i, tr in enumerate(trs) if i != 1] == [x for i, x in enumerate(c.prover_states) if i != 1]
    with pytest.raises(bpp.ProofError):
        bpp.RangeProof.prove_with_rng(trs[1], wrong[1], c.witnesses[1], c.ext[1], advance=True)
    assert (trs[1].label, trs[1].state) == before


def test_self_check_remake_and_failure(bpp, engine, opt):
    """"prove_check" = 1 with the test knob that alters one proof in the host copy: altered once, the proof is made again and the
    state returned is the remade proof's (the same bytes); altered twice, the item fails with BPP_ERR_SELF_CHECK and its row keeps
    the prefill while the others are written"""
    c = prove_case(bpp, engine, 1)
    opt("prove_check", 1)
    engine.set_option("prove_check_tamper", 3)  # the m = 4 item of the call
    rc, codes, proofs, rows = raw_prove_states(bpp, c, c.statements)
    assert rc == 0 and codes == [0] * 5 and proofs == c.raw and rows == c.prover_states
    assert engine.prove_check_stats()["remade"] >= 1
    engine.set_option("prove_check_tamper", 3)
    engine.set_option("prove_check_tamper_times", 2)
    rc, codes, proofs, rows = raw_prove_states(bpp, c, c.statements)
    assert rc == -5 and codes == [0, 0, -5, 0, 0]
    assert rows[2] == bytes([PREFILL]) * 203
    assert [r for i, r in enumerate(rows) if i != 2] == [r for i, r in enumerate(c.prover_states) if i != 2]


# --------------------------------------------------------------------------------------------------------------- 5. composition
def test_prover_state_plus_the_responses_is_the_verifier_state(bpp, engine):
    c = verify_case(bpp, engine, 1)
    for i, raw in enumerate(c.raw):
        tr = bpp.Transcript.from_state(c.prover_states[i])
        assert tr.state != c.verifier_states[i]  # the two sides end in different states, as in the reference
        tr.append_message(b"r1", raw[1 + 32 + 96:1 + 32 + 128])
        tr.append_message(b"s1", raw[1 + 32 + 128:1 + 32 + 160])
        tr.append_message(b"d1", raw[1:33])
        assert tr.state == c.verifier_states[i], i


def test_a_range_proof_inside_a_larger_protocol(bpp, engine):
    """context, then prove / verify with advance=True, then a challenge from the same transcript: the oracle's bytes on both sides"""
    c = verify_case(bpp, engine, 1)
    st, ext = c.o_statements[0], c.ext[0]
    o_proof = O.RangeProof.from_bytes(c.raw[0])
    # (the transcript O.prove_with_rng left when the shared case made this proof: restored from its bytes, not proved again)
    o_prover = M.Transcript()
    o_prover.strobe = M.Strobe128()
    o_prover.strobe.state = bytearray(c.prover_states[0][:200])
    o_prover.strobe.pos, o_prover.strobe.pos_begin, o_prover.strobe.cur_flags = c.prover_states[0][200:203]
    want_prover = o_prover.challenge_bytes(b"after", 32)
    o_verifier = o_transcript()
    O.verify([o_verifier], [st], [o_proof], 0)
    want_verifier = o_verifier.challenge_bytes(b"after", 32)
    assert want_prover != want_verifier

    tr = bpp.Transcript.new(LABEL)
    tr.append_message(CTX_LABEL, CTX)
    proof = bpp.RangeProof.prove_with_rng(tr, c.statements[0], c.witnesses[0], ext, advance=True)
    assert proof.to_bytes() == c.raw[0]
    assert tr.challenge_bytes(b"after", 32) == want_prover
    tv = bpp.Transcript.new(LABEL)
    tv.append_message(CTX_LABEL, CTX)
    bpp.RangeProof.verify_batch([tv], [c.statements[0]], [proof], bpp.VerifyAction.VerifyOnly, advance=True)
    assert tv.challenge_bytes(b"after", 32) == want_verifier
    assert tv.state == o_verifier.strobe.to_bytes()


# ------------------------------------------------------------------------------------------------- 6. the default is as before
def test_without_advance_nothing_changes(bpp, engine):
    c = verify_case(bpp, engine, 1)
    A = bpp.VerifyAction
    trs = [bpp.Transcript.from_state(o_transcript().strobe.to_bytes()) for _ in range(5)]
    labelled = bpp.Transcript.new(LABEL)
    before = [(tr.label, tr.state) for tr in trs]
    assert masks_of(bpp.RangeProof.verify_batch(trs, c.statements, c.proofs, A.RecoverAndVerify, chunk=0)) == c.masks
    got = bpp.RangeProof.prove_batch_mixed(trs, c.statements, c.witnesses, c.ext)
    assert [p.to_bytes() for p in got] == c.raw
    assert bpp.RangeProof.prove_with_rng(trs[0], c.statements[0], c.witnesses[0], c.ext[0]).to_bytes() == c.raw[0]
    assert [(tr.label, tr.state) for tr in trs] == before
    with pytest.raises(bpp.ProofError):  # (the proofs are bound to the context: a label alone is another transcript)
        bpp.RangeProof.verify_batch([labelled], [c.statements[0]], [c.proofs[0]], A.VerifyOnly)
    assert (labelled.label, labelled.state) == (LABEL, None)
    # the C entry points refuse a null state buffer instead of guessing
    eng = c.params.engine
    items, keep = bpp.RangeProof._items(trs, c.statements, c.proofs)
    err = ctypes.create_string_buffer(256)
    assert eng.lib.bpp_verify_batch_states(eng.ctx, c.params.handle, items, 5, 0, 0, None, None, None, err, 256) == 2
