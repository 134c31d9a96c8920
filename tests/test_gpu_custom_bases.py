"""GPU tests of caller-supplied Pedersen bases (bpp_params_create's h_base32 / g_bases32, api.PedersenGens(t, h, gs)): everything
the engine derives from them -- the generator table's tail and its split copy, the prover's fixed-base windows, the constant-time
lines, the transcript's copy of the encodings, the registry entry other contexts share -- against the oracle under the same bases
(tests/helpers.py: oracle_pedersen_gens).  Every witness has a blinding of its own per generator, so a swapped or a stale default
base changes a commitment, a proof byte or a verdict.  Everything compared is exact."""
import pytest

from oracle.pyref import curve as C
from oracle.pyref import merlin as M
from oracle.pyref import protocol as O
from tests import helpers as H
from tests.helpers import sb

pytestmark = pytest.mark.gpu

# key -> (bit length, aggregation factors, extension degree, base set)
CONFIGS = {"n8-random": (8, [1, 2], 2, "random"), "n8-edge": (8, [1, 2], 2, "edge"), "n64-random": (64, [1], 1, "random")}
KEYS = list(CONFIGS)
_CACHE, _ORACLE = {}, {}


def _cfg(bpp, engine, key):
    """(the batch under the caller's bases, the same recipe under the default bases), both bound to the session engine and alive
    side by side: two parameter sets of one (n, m, t)"""
    if key not in _CACHE:
        n, agg, t, which = CONFIGS[key]
        pc = H.custom_pedersen_gens(t, which, tag=key.encode())
        seed = b"custom-" + key.encode()
        _CACHE[key] = (H.make_batch(bpp, engine, n, agg, t, seed=seed, pc_gens=pc), H.make_batch(bpp, engine, n, agg, t, seed=seed))
    return _CACHE[key]


def _oracle(key, c, action):
    if (key, action) not in _ORACLE:
        _ORACLE[(key, action)] = H.oracle_verify_trace(c, action=action)
    return _ORACLE[(key, action)]


def _kind(bpp, call):
    try:
        call()
        return 0
    except bpp.ProofError as e:
        return int(e.kind)


def _oracle_kind(label, statements, proofs):
    try:
        O.verify([M.Transcript(label) for _ in proofs], statements, proofs, O.VERIFY_ONLY)
        return 0
    except O.ProofError as e:
        return int(e.kind)


def _witnesses(bpp, c):
    return [bpp.RangeWitness.init([bpp.CommitmentOpening.new(o.v, [sb(r) for r in o.r]) for o in w.openings]) for w in c.o_witnesses]


def _prove(bpp, c):
    got = bpp.RangeProof.prove_batch_mixed(c.transcripts(), c.statements_private, _witnesses(bpp, c), c.o_ext)
    assert not any(isinstance(g, Exception) for g in got), got
    return [g.to_bytes() for g in got]


def _commit_cases(c):
    """(value, blinding factors): 0, 2^64 - 1 and every witness value, each with one blinding factor and with t"""
    out = []
    for i, v in enumerate([0, 2**64 - 1] + [o.v for w in c.o_witnesses for o in w.openings]):
        r = [H.msm_hashed(b"custom-blind-%d" % i, k) for k in range(c.t)]
        out += [(v, r[:1]), (v, r)]
    return out


def _check_commits(c):
    cases = _commit_cases(c)
    for nb in sorted({len(r) for _, r in cases}):
        sel = [(v, r) for v, r in cases if len(r) == nb]
        got = c.params.commit_many([v for v, _ in sel], [[sb(x) for x in r] for _, r in sel])
        assert got == [c.o_params.pc_gens.commit(v, r).compress() for v, r in sel], nb


def _check_verify(bpp, key, c, actions=(0, 1, 2)):
    for action in actions:
        want, _ = _oracle(key, c, action)
        sts = c.statements_private if action else c.statements_public
        got = bpp.RangeProof.verify_batch(c.transcripts(), sts, c.proofs, bpp.VerifyAction(action))
        assert [m.blindings() if m is not None else None for m in got] == want, action


@pytest.mark.parametrize("key", KEYS)
def test_export_and_commitments(bpp, engine, opt, key):
    c, d = _cfg(bpp, engine, key)
    pc = c.o_params.pc_gens
    assert c.params.h_base_compressed() == pc.h_base_compressed and c.params.g_bases_compressed() == pc.g_base_compressed_vec
    assert c.params.h_base_compressed() != d.params.h_base_compressed() and c.params.g_bases_compressed()[0] != d.params.g_bases_compressed()[0]
    assert c.params.gi_base_compressed() == d.params.gi_base_compressed() and c.params.hi_base_compressed() == d.params.hi_base_compressed()
    _check_commits(c)       # the uniform-access lines (fb_ct)
    opt("ct", 0)
    _check_commits(c)       # the fixed-base windows (fb_ped)
    # the statements' commitments are the oracle's under these bases
    for st, ow in zip(c.o_statements_public, c.o_witnesses):
        got = c.params.commit_many([o.v for o in ow.openings], [[sb(x) for x in o.r] for o in ow.openings])
        assert got == st.commitments_compressed


@pytest.mark.parametrize("key", KEYS)
def test_prover_bytes(bpp, engine, opt, key):
    c, _ = _cfg(bpp, engine, key)
    want = [p.to_bytes() for p in c.o_proofs]
    for ct in (1, 0, 2):
        opt("ct", ct)
        assert _prove(bpp, c) == want, ct
    opt("ct", -1)
    sts, proofs = bpp.RangeProof.prove_openings(c.transcripts(), _witnesses(bpp, c), [s.minimum_value_promises for s in c.o_statements_private],
                                                [s.seed_nonce for s in c.statements_private], c.o_ext, c.params)
    assert not any(isinstance(p, Exception) for p in proofs), proofs
    assert [p.to_bytes() for p in proofs] == want
    assert [s.commitments_compressed for s in sts] == [s.commitments_compressed for s in c.o_statements_public]


@pytest.mark.parametrize("key", KEYS)
def test_verifier_masks_and_intermediates(bpp, engine, key):
    c, _ = _cfg(bpp, engine, key)
    _check_verify(bpp, key, c)
    _, tr = _oracle(key, c, 0)
    rb = bpp.ResidentBatch(c.transcripts(), c.statements_public, c.proofs)
    assert rb.verify(bpp.VerifyAction.VerifyOnly, chunk=0) == [None] * len(c.proofs)
    static = b"".join(sb(g) + sb(h) for g, h in zip(tr["gi"], tr["hi"])) + b"".join(sb(x) for x in tr["g"]) + sb(tr["h"])
    assert rb.trace(4) == static
    assert rb.trace(5) == b"".join(sb(x) for x in tr["dynamic_scalars"])
    assert rb.trace(6) == tr["msm_result"] == bytes(32)
    rb.close()


def _cross(bpp, src, dst):
    """src's proofs and commitments under dst's parameters: (product outcome, oracle outcome)"""
    sts = [bpp.RangeStatement.init(dst.params, s.commitments_compressed, s.minimum_value_promises, None) for s in src.statements_public]
    got = _kind(bpp, lambda: bpp.RangeProof.verify_batch(src.transcripts(), sts, src.proofs, bpp.VerifyAction.VerifyOnly))
    return got, _oracle_kind(src.label, H.restate(src, dst.o_params), src.o_proofs)


@pytest.mark.parametrize("key", KEYS)
def test_proofs_do_not_verify_under_the_other_bases(bpp, engine, key):
    c, d = _cfg(bpp, engine, key)
    for src, dst in ((c, d), (d, c)):
        got, want = _cross(bpp, src, dst)
        assert got == want == int(bpp.ProofErrorKind.VerificationFailed)
    _check_verify(bpp, key, c, actions=(0,))


def test_two_parameter_sets_of_one_shape_side_by_side(bpp, engine):
    """default and custom parameters of (8, 2, 2) alive in one context, calls interleaved: each result is its own oracle's; then the
    custom set shared into a second context"""
    key = "n8-random"
    c, d = _cfg(bpp, engine, key)
    want_c, want_d = [p.to_bytes() for p in c.o_proofs], [p.to_bytes() for p in d.o_proofs]
    assert want_c != want_d
    for _ in range(2):
        _check_commits(c)
        _check_commits(d)
        assert _prove(bpp, d) == want_d
        assert _prove(bpp, c) == want_c
        for x in (c, d, c):
            got = bpp.RangeProof.verify_batch(x.transcripts(), x.statements_private, x.proofs, bpp.VerifyAction.RecoverAndVerify)
            assert [m.blindings() if m is not None else None for m in got] == [[sb(v) for v in m] if m is not None else None for m in x.expected_masks]
    eng2 = bpp.Engine(0)
    shared = c.params.share(eng2)
    try:
        sts = [bpp.RangeStatement.init(shared, s.commitments_compressed, s.minimum_value_promises, s.seed_nonce) for s in c.statements_private]
        got = bpp.RangeProof.verify_batch(c.transcripts(), sts, c.proofs, bpp.VerifyAction.RecoverAndVerify)
        assert [m.blindings() if m is not None else None for m in got] == _oracle(key, c, 1)[0]
        bad = [bpp.RangeStatement.init(shared, s.commitments_compressed, s.minimum_value_promises, None) for s in d.statements_public]
        assert _kind(bpp, lambda: bpp.RangeProof.verify_batch(d.transcripts(), bad, d.proofs, bpp.VerifyAction.VerifyOnly)) == \
            int(bpp.ProofErrorKind.VerificationFailed)
        cases = _commit_cases(c)[:4]
        assert [shared.commit(v, [sb(x) for x in r]) for v, r in cases] == [c.o_params.pc_gens.commit(v, r).compress() for v, r in cases]
    finally:
        shared.close()
        eng2.close()
    _check_verify(bpp, key, c, actions=(0,))  # the first holder's reference is untouched


def test_prover_self_check_on_custom_bases(bpp, engine, opt):
    c, _ = _cfg(bpp, engine, "n8-edge")
    opt("prove_check", 1)
    s0 = engine.prove_check_stats()
    assert _prove(bpp, c) == [p.to_bytes() for p in c.o_proofs]
    s1 = engine.prove_check_stats()
    assert {k: s1[k] - s0[k] for k in s1} == dict(calls=1, proofs=len(c.o_proofs), batch_failures=0, remade=0, failed=0)


def test_joint_final_check_on_custom_bases(bpp, engine, opt):
    """two groups (chunk = 1) under "verify_joint": accepted jointly; the default-base proofs fall back and fail group by group"""
    c, d = _cfg(bpp, engine, "n8-random")
    opt("verify_joint", 1)
    rb = bpp.ResidentBatch(c.transcripts(), c.statements_public, c.proofs)
    s0 = engine.verify_joint_stats()
    rb.verify_only(chunk=1)
    s1 = engine.verify_joint_stats()
    assert rb.shape()["groups"] == 2
    assert {k: s1[k] - s0[k] for k in s1} == dict(calls=1, accepted=1, fallbacks=0, fallback_all_ok=0)
    assert rb.trace(8) == bytes(32)
    rb.close()
    sts = [bpp.RangeStatement.init(c.params, s.commitments_compressed, s.minimum_value_promises, None) for s in d.statements_public]
    rb = bpp.ResidentBatch(d.transcripts(), sts, d.proofs)
    assert _kind(bpp, lambda: rb.verify_only(chunk=1)) == int(bpp.ProofErrorKind.VerificationFailed)
    s2 = engine.verify_joint_stats()
    assert {k: s2[k] - s1[k] for k in s2} == dict(calls=1, accepted=0, fallbacks=1, fallback_all_ok=0)
    rb.close()


def test_plain_msm_on_custom_bases(bpp, engine, opt):
    """ "msm_plain" = 1: the B1 entry points over the caller's bases give the engine's own commitments; "verify_check" = 1 confirms the
    rejection under the other bases on the plain kernels and leaves the verdicts as they are"""
    key = "n8-edge"
    c, d = _cfg(bpp, engine, key)
    opt("msm_plain", 1)
    pc = c.o_params.pc_gens
    pts = [pc.h_base_compressed] + pc.g_base_compressed_vec
    for v, r in _commit_cases(c):
        if len(r) == c.t:
            assert engine.msm_vartime([sb(v)] + [sb(x) for x in r], pts) == c.params.commit(v, [sb(x) for x in r])
    assert engine.msm_last_plan()["plain"]
    _check_verify(bpp, key, c)
    opt("verify_check", 1)
    s0 = engine.verify_check_stats()
    _check_verify(bpp, key, c, actions=(0,))
    got, want = _cross(bpp, d, c)
    assert got == want == int(bpp.ProofErrorKind.VerificationFailed)
    s1 = engine.verify_check_stats()
    delta = {k: s1[k] - s0[k] for k in s1}
    assert delta["rechecked_groups"] == 1 and delta["confirmed"] == 1 and delta["overturned"] == delta["undecided"] == 0, delta
