"""GPU suite: the verifier's scalar stage (PASS 2 of csrc/kernels_verify.h: k_scalars_shared, the lanes kernel, the table
kernels, k_static_gemm, the column reductions, the mask-recovery kernel with its batch inversion) under CHOSEN scalars.

Every other test feeds that stage hash output; the places where the device's Z_l arithmetic (csrc/scalar.h: Montgomery form with
R = 2^261, nine 29-bit limbs, lazy representatives below 2l, sc18_redc over summed products) can be wrong are a limb of 29 one-bits,
a result that needs the last conditional subtraction, a square or an inverse that is 1 or l-1, z^2 - z = 0, y^(mn) = 1.  Two public
handles reach the stage with such values:

  * bpp_verify_batch_with_challenges takes y, z, e_j, e from the caller.  An honest (oracle) prover run under forced challenges
    gives a proof that verifies under them exactly when every PASS 2 scalar and every MSM scalar is right
    (tests/helpers.py: edge_challenge_families; tests/test_verify_edges_host.py holds the families to the oracle);
  * proof bytes and statements carry r1, s1, d1 and the u64 promises: here the batch is rejected, and the parity traces
    (weights, static scalars, dynamic scalars, the compressed non-identity sum) are the oracle's.

Shapes are the smallest at which each loop still runs: (n, m, t) = (8,1,1) three rounds and mask recovery; (8,2,2) four rounds, the
d_sum loop once, two d1; (16,4,1) six rounds, the d_sum loop twice, z powers across parties, and -- 64 generator pairs -- the only
one of the three whose generator columns can be summed inside k_scalars_lanes (fused_columns / lazy_columns) or taken from the
matrix product (static_gemm with tables_wave = 0); at 8 and 16 pairs those options leave the per-proof rows (engine.hip:
plan_lanes)."""
import time

import pytest

from oracle import cport
from oracle.pyref import curve as C
from oracle.pyref import merlin as M
from oracle.pyref import protocol as O
from tests import helpers as H
from tests.helpers import LABEL, sb

pytestmark = pytest.mark.gpu

L = C.L
S811, S822, S1641 = (8, 1, 1, None), (8, 2, 2, None), (16, 4, 1, 4)
SHAPES = {S811: H.EDGE_POSITION_CLASSES + ("all_edge",), S822: H.EDGE_POSITION_CLASSES + ("all_edge",), S1641: ("y", "z", "all_edge")}
SHAPE_FAMILY = [(s, f) for s, fams in SHAPES.items() for f in fams]
_ids = lambda s: "n%d-m%d-t%d" % s[:3]


class _Shape:
    """the families of one shape bound to device parameters: per case the statement (private for m == 1) and the proof"""

    def __init__(self, bpp, engine, shape):
        n, m, t, m_max = shape
        t0 = time.perf_counter()
        self.families = H.edge_challenge_families(n, m, t, m_max, only=SHAPES[shape])
        self.oracle_seconds = time.perf_counter() - t0
        self.m, self.t = m, t
        self.action = bpp.VerifyAction.RecoverAndVerify if m == 1 else bpp.VerifyAction.VerifyOnly
        self.params = bpp.RangeParameters.init(n, m_max or m, bpp.create_pedersen_gens_with_extension_degree(t), engine=engine)
        self.bpp = bpp
        self._bound = {}

    def bind(self, c, private=None):
        private = (self.m == 1) if private is None else private
        key = (c.name, private)
        if key not in self._bound:
            st = c.o_statement_private
            nonce = sb(st.seed_nonce) if private and st.seed_nonce is not None else None
            self._bound[key] = (self.bpp.RangeStatement.init(self.params, list(st.commitments_compressed), st.minimum_value_promises, nonce),
                                self.bpp.RangeProof.from_bytes(c.o_proof.to_bytes()))
        return self._bound[key]

    def cases(self):
        return [c for fam in H.EDGE_POSITION_CLASSES + ("all_edge",) if fam in self.families for c in self.families[fam]]

    def run(self, cases, action=None, chunk=0, challenges=None, private=None):
        """-> masks as lists of 32-byte strings | None per case, or the name of the ProofErrorKind"""
        action = self.action if action is None else action
        bound = [self.bind(c, private) for c in cases]
        chal = challenges if challenges is not None else [c.challenges[0] for c in cases]
        try:
            got = self.bpp.verify_batch_with_challenges([b[0] for b in bound], [b[1] for b in bound], chal,
                                                        [c.rng_outputs[0] for c in cases], action, chunk=chunk)
        except self.bpp.ProofError as e:
            return self.bpp.ProofErrorKind(e.kind).name
        return [m.blindings() if m is not None else None for m in got]


@pytest.fixture(scope="module")
def shapes(bpp, engine):
    """every case of every shape, made once (Python proving is the larger share of this module's time)"""
    out = {s: _Shape(bpp, engine, s) for s in SHAPES}
    print("\noracle proving: " + ", ".join("%s %d cases %.1f s" % (_ids(s), len(out[s].cases()), out[s].oracle_seconds) for s in SHAPES))
    yield out
    for s in out.values():
        s.params.close()


# ---- a. every case alone -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,family", SHAPE_FAMILY, ids=["%s-%s" % (_ids(s), f) for s, f in SHAPE_FAMILY])
def test_each_case_alone(shapes, shape, family):
    """one proof per call: accepted, and for m == 1 the oracle's masks (the witness's blinding factors) come back"""
    sh = shapes[shape]
    bad = []
    for c in sh.families[family]:
        assert c.oracle_error is None, c.name
        got = sh.run([c])
        if got != c.expected_masks:
            bad.append((c.name, got if isinstance(got, str) else "masks differ"))
    assert not bad, bad


# ---- b. one batch, every kernel form -------------------------------------------------------------------------------------------

FORMS = {
    "default": ({}, 0),
    "tables_wave=0": ({"tables_wave": 0}, 0),
    "tables_wave=1": ({"tables_wave": 1}, 0),
    "static_gemm=0": ({"static_gemm": 0}, 0),
    "static_gemm=1": ({"static_gemm": 1}, 0),
    # the matrix product is taken only over the tables of k_scalars_shared (plan_lanes), which small inputs get with tables_wave = 0
    "static_gemm=1,tables_wave=0": ({"static_gemm": 1, "tables_wave": 0}, 0),
    "fused=1,lazy=1": ({"static_gemm": 0, "fused_columns": 1, "lazy_columns": 1}, 0),
    "fused=1,lazy=0": ({"static_gemm": 0, "fused_columns": 1, "lazy_columns": 0}, 0),
    "fused=0,lazy=0": ({"static_gemm": 0, "fused_columns": 0, "lazy_columns": 0}, 0),
    "chunk=24": ({}, 24),  # 103 = 4 * 24 + 7, 35 = 24 + 11
}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("shape", list(SHAPES), ids=_ids)
def test_one_batch_in_every_kernel_form(shapes, opt, shape, form):
    """all cases of a shape as ONE call.  (8,1,1) and (8,2,2) hold 103 proofs each -- every (position class, value) but y = 1, and
    the two all-edge rows -- which is more than the 70 asked for: two wavefronts of proofs, the second part-filled, without a
    second seed.  (16,4,1) holds 35."""
    sh = shapes[shape]
    cases = sh.cases()
    assert len(cases) == (35 if shape == S1641 else 103) and (shape == S1641 or len(cases) >= 70)
    options, chunk = FORMS[form]
    assert chunk == 0 or len(cases) % chunk
    for k, v in options.items():
        opt(k, v)
    got = sh.run(cases, chunk=chunk)
    assert not isinstance(got, str), got
    bad = [c.name for c, g in zip(cases, got) if [g] != c.expected_masks]
    assert not bad, bad


# ---- c. every challenge is consumed --------------------------------------------------------------------------------------------

def _bumped(v):
    """value + 1 mod l -- except at l-1, where that is 0: a zero challenge is refused by a check of its own before any arithmetic
    (test_verify_with_external_challenges), which says nothing about the position being used.  l-1 becomes l-2 instead (not 1: y = 1
    is SURVEY q10)"""
    return (v + 1) % L if v != L - 1 else L - 2


@pytest.mark.parametrize("shape", list(SHAPES), ids=_ids)
def test_every_challenge_position_is_consumed(shapes, shape):
    """the alternating all-edge case with ONE position moved by one: rejected, whichever position"""
    sh = shapes[shape]
    c = sh.families["all_edge"][1]
    assert c.name == "alternating" and set(c.values) == {1, L - 1}
    assert sh.run([c], action=sh.bpp.VerifyAction.VerifyOnly, private=False) == [None]
    verdicts = {}
    for k, v in enumerate(c.values):
        row = list(c.values)
        row[k] = _bumped(v)
        assert row[k] not in (0, v) and not (k == 0 and row[k] == 1)
        verdicts[k] = sh.run([c], action=sh.bpp.VerifyAction.VerifyOnly, private=False, challenges=[[sb(x) for x in row]])
        if v == L - 1:  # and the literal value + 1 = 0
            row[k] = 0
            assert sh.run([c], action=sh.bpp.VerifyAction.VerifyOnly, private=False, challenges=[[sb(x) for x in row]]) == "VerificationFailed", k
    assert verdicts == {k: "VerificationFailed" for k in range(len(c.values))}


def test_recovered_masks_move_with_every_challenge(shapes):
    """RecoverOnly at (8,1,1): the recovery formula (src/range_proof.rs:941-969) reads y, z, every e_j and e, so the masks under a
    row with one position moved are not the witness's; they are what the oracle recovers under that row"""
    sh = shapes[S811]
    A = sh.bpp.VerifyAction.RecoverOnly
    c = sh.families["all_edge"][1]
    assert sh.run([c], action=A) == c.witness_masks
    bad = []
    for k, v in enumerate(c.values):
        row = list(c.values)
        row[k] = _bumped(v)
        want, err, _ = H.oracle_verify_forced(c, row, 2)
        assert err is None and want != c.witness_masks and want[0] is not None, k
        got = sh.run([c], action=A, challenges=[[sb(x) for x in row]])
        if got != want:
            bad.append((k, got if isinstance(got, str) else "masks differ"))
    assert not bad, bad


# ---- 4. y = 1 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,m,t", [(8, 1, 1), (8, 2, 2)])
def test_y_one_is_rejected(bpp, engine, n, m, t):
    """the engine inverts [e_j.., y, y - 1] as one product (k_scalars_shared, as the reference's batch_invert call),
    the oracle per element with inverse(0) = 0.  At y = 1 they differ in e_j^-1, and both reject: y_sum is wrong in either.
    Nothing is asserted about the masks of RecoverOnly there."""
    c = H.edge_y_one_case(n, m, t)
    assert c.values[0] == 1 and c.oracle_error is not None and c.oracle_error.kind == O.VERIFICATION_FAILED
    params = bpp.RangeParameters.init(n, m, bpp.create_pedersen_gens_with_extension_degree(t), engine=engine)
    st = c.o_statement_private
    for action, nonce in ((bpp.VerifyAction.VerifyOnly, None), (bpp.VerifyAction.RecoverAndVerify, st.seed_nonce)):
        stp = bpp.RangeStatement.init(params, list(st.commitments_compressed), st.minimum_value_promises, sb(nonce) if nonce is not None else None)
        with pytest.raises(bpp.ProofError) as e:
            bpp.verify_batch_with_challenges([stp], [bpp.RangeProof.from_bytes(c.o_proof.to_bytes())], c.challenges, c.rng_outputs, action, chunk=0)
        assert e.value.kind == bpp.ProofErrorKind.VerificationFailed
    params.close()


# ---- d. edge responses on the ordinary path, with traces -----------------------------------------------------------------------

def _response_mutants(raw, t):
    """(name, proof bytes): r1, s1 and each d1[k] overwritten, one field at a time, with every edge scalar and with 0; then all
    fields l-1, all fields 0.  Wire format: t, d1[t], A, A1, B, r1, s1, (L, R)*"""
    fields = [("r1", 1 + 32 * t + 96), ("s1", 1 + 32 * t + 128)] + [("d1[%d]" % k, 1 + 32 * k) for k in range(t)]
    out = []
    for fname, off in fields:
        for vname, v in H.EDGE_SCALARS + [("0", 0)]:
            assert raw[off:off + 32] != sb(v)
            out.append(("%s=%s" % (fname, vname), fname, raw[:off] + sb(v) + raw[off + 32:]))
    for vname, v in (("l-1", L - 1), ("0", 0)):
        r = bytearray(raw)
        for _, off in fields:
            r[off:off + 32] = sb(v)
        out.append(("all=%s" % vname, "all", bytes(r)))
    return out


def _oracle_traces(c, o_statements, raws):
    """the oracle's VerifyOnly of `raws` as one batch -> (error kind | None, weights, statics, dynamic scalars, result) in the layouts
    of BPP_TRACE 3, 4, 5, 6 for one group"""
    tr = {}
    kind = None
    try:
        O.verify([M.Transcript(c.label) for _ in raws], o_statements, [O.RangeProof.from_bytes(r) for r in raws], 0, trace=tr)
    except O.ProofError as e:
        kind = e.kind
    statics = b"".join(sb(a) + sb(b) for a, b in zip(tr["gi"], tr["hi"])) + b"".join(sb(x) for x in tr["g"]) + sb(tr["h"])
    return kind, b"".join(sb(w) for w in tr["weights"]), statics, b"".join(sb(x) for x in tr["dynamic_scalars"]), tr["msm_result"]


def _device_traces(bpp, c, statements, raws, chunk=0):
    rb = bpp.ResidentBatch([bpp.Transcript.new(c.label) for _ in raws], statements, [bpp.RangeProof.from_bytes(r) for r in raws])
    try:
        kind = None
        try:
            rb.verify(bpp.VerifyAction.VerifyOnly, chunk=chunk)
        except bpp.ProofError as e:
            kind = int(e.kind)
        return kind, rb.trace(3), rb.trace(4), rb.trace(5), rb.trace(6)
    finally:
        rb.close()


RESPONSE_SHAPES = [(8, 1, 2), (8, 2, 1)]


@pytest.fixture(scope="module")
def responses(bpp, engine):
    """per shape: the valid batch of one proof, its mutants, and the oracle's traces of every mutant alone and of all together"""
    out = {}
    for n, m, t in RESPONSE_SHAPES:
        c = H.make_batch(bpp, engine, n, [m], t, seed=b"edge-resp-%d-%d" % (m, t))
        mutants = _response_mutants(c.o_proofs[0].to_bytes(), t)
        assert len(mutants) == (2 + t) * 18 + 2
        raws = [r for _, _, r in mutants]
        alone = [_oracle_traces(c, c.o_statements_public, [r]) for r in raws]
        joint = _oracle_traces(c, c.o_statements_public * len(raws), raws)
        out[(n, m, t)] = (c, mutants, alone, joint)
    yield out
    for c, _, _, _ in out.values():
        c.params.close()


@pytest.mark.parametrize("lazy", [0, 1])
@pytest.mark.parametrize("shape", RESPONSE_SHAPES, ids=_ids)
def test_edge_responses_in_one_batch(bpp, opt, responses, shape, lazy):
    """all mutants of a shape in one resident batch: rejected, and weights, static scalars, dynamic scalars and the compressed
    non-identity sum are the oracle's"""
    c, mutants, _, want = responses[shape]
    assert want[0] == O.VERIFICATION_FAILED and want[4] != bytes(32)
    opt("lazy_columns", lazy)
    got = _device_traces(bpp, c, c.statements_public * len(mutants), [r for _, _, r in mutants])
    assert got[0] == int(bpp.ProofErrorKind.VerificationFailed)
    for what, g, w in zip(("weights", "static scalars", "dynamic scalars", "msm result"), got[1:], want[1:]):
        assert g == w, what


RESPONSE_FIELDS = [(s, f) for s in RESPONSE_SHAPES for f in ["r1", "s1"] + ["d1[%d]" % k for k in range(s[2])] + ["all"]]


@pytest.mark.parametrize("shape,field", RESPONSE_FIELDS, ids=["%s-%s" % (_ids(s), f) for s, f in RESPONSE_FIELDS])
def test_edge_responses_alone(bpp, responses, shape, field):
    """each mutant as a batch of its own, so that a failure names the field and the value"""
    c, mutants, alone, _ = responses[shape]
    picked = [(name, raw, want) for (name, f, raw), want in zip(mutants, alone) if f == field]
    assert len(picked) == (2 if field == "all" else 18)
    bad = []
    for name, raw, want in picked:
        assert want[0] == O.VERIFICATION_FAILED and want[4] != bytes(32), name
        got = _device_traces(bpp, c, c.statements_public, [raw])
        if got[0] != int(bpp.ProofErrorKind.VerificationFailed):
            bad.append((name, "verdict", got[0]))
        bad += [(name, what) for what, g, w in zip(("weights", "static scalars", "dynamic scalars", "msm result"), got[1:], want[1:]) if g != w]
    assert not bad, bad


# ---- e. edge promises ----------------------------------------------------------------------------------------------------------

PROMISES = [None, 0, 1, 2**29 - 1, 2**29, 2**32 - 1, 2**32, 2**58 - 1, 2**58, 2**63, 2**64 - 1]


def _c_prove(cp, seed, values, mins):
    rng = H.Prng(seed)
    blinds = [[sb(O.random_not_zero(rng))] for _ in values]
    proof, commitments = cp.prove(LABEL, values, blinds, mins, None, rng.fill_bytes(32 * 10))
    return proof, commitments


@pytest.fixture(scope="module")
def promise_setup(bpp, engine):
    cp = cport.Params(64, 2, 1)
    params = bpp.RangeParameters.init(64, 2, bpp.create_pedersen_gens_with_extension_degree(1), engine=engine)
    yield cp, params
    params.close()
    cp.close()


def _promise_parity(bpp, cp, params, proof, commitments, mins):
    """-> None, or what differs between the engine and the C oracle for this statement"""
    rc, _, want = cp.verify([{"proof": proof, "commitments": commitments, "min_values": mins, "seed_nonce": None, "label": LABEL}], 0,
                            want_trace=True)
    st = bpp.RangeStatement.init(params, commitments, mins, None)
    c = H.Case()
    c.label = LABEL
    got = _device_traces(bpp, c, [st], [proof])
    if (got[0] or 0) != rc:
        return "verdict %r, oracle %r" % (got[0], rc)
    for what, g, w in zip(("static scalars", "dynamic scalars", "msm result"), got[2:], (want["static_scalars"], want["dynamic_scalars"], want["msm_result"])):
        if g != w:
            return what
    return rc


@pytest.mark.parametrize("where", ["first", "last", "both"])
def test_edge_promises(bpp, promise_setup, where):
    """one valid 64-bit proof of two parties restated with promises at the limb and word boundaries of a u64 turned scalar (the h
    scalar is the one they move; they also enter the transcript): verdict -- most are rejections -- and traces 4, 5, 6 are the C
    oracle's on the same statement"""
    cp, params = promise_setup
    values = [0x0123456789ABCDEF, 0xFEDCBA9876543210]
    mins = [values[0] // 3, values[1] // 3]
    proof, commitments = _c_prove(cp, b"edge-promise", values, mins)
    assert _promise_parity(bpp, cp, params, proof, commitments, mins) == 0
    bad, verdicts = [], []
    for p in PROMISES:
        restated = [p if (j == 0 and where != "last") or (j == 1 and where != "first") else mins[j] for j in range(2)]
        r = _promise_parity(bpp, cp, params, proof, commitments, restated)
        if isinstance(r, str):
            bad.append((p, r))
        verdicts.append(r)
    assert not bad, bad
    assert set(verdicts) == {O.VERIFICATION_FAILED}  # none of the eleven is this proof's own promise


def test_largest_promise_on_a_valid_proof(bpp, promise_setup):
    """v = vmin = 2^64 - 1 at either party, proved by the oracle: accepted by both"""
    cp, params = promise_setup
    for values, mins in (([2**64 - 1, 12345], [2**64 - 1, None]), ([12345, 2**64 - 1], [17, 2**64 - 1]), ([2**64 - 1] * 2, [2**64 - 1] * 2)):
        proof, commitments = _c_prove(cp, b"edge-promise-max", values, mins)
        assert _promise_parity(bpp, cp, params, proof, commitments, mins) == 0, mins
