"""GPU tests of the three compiled forms of the ristretto255 decoder against the corpus of tests/ristretto_corpus.py, whose
members one condition of RFC 9496 4.3.1 alone refuses (tests/test_ristretto_corpus.py pins the corpus and the HOST compile).

  k_decompress_plain (ristretto_decompress): bpp_msm_vartime, bpp_msm_ct, bpp_precomp_create, the dynamic points of
      bpp_msm_mixed, the Pedersen bases of bpp_params_create;
  k_decompress (ristretto_decompress_lean) with its limb-major spill array: the proof points of every verification;
  the same kernel without the array: the statement's commitments at upload, and every point under BPP_DECOMPRESS_SPILL=0
      (read once per process: a child process).

Everything compared is exact: bytes, verdicts, error kinds."""
import hashlib
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle.pyref import curve as C
from oracle.pyref import merlin as M
from oracle.pyref import protocol as O
from tests import ristretto_corpus as R
from tests.helpers import LABEL, make_oracle_batch, attach_product, sb

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, VERIFICATION_FAILED, INVALID_ARGUMENT = 0, 1, 2
VALID = [(name, b) for name, b in R.CORPUS if R.classify(b) == "valid"]
INVALID = [(name, b) for name, b in R.CORPUS if R.classify(b) != "valid"]
NAMED_VALID = [(name, b) for name, b in R.NAMED if R.classify(b) == "valid"]
NAMED_INVALID = [(name, b) for name, b in R.NAMED if R.classify(b) != "valid"]
T_NEGATIVE = R.enc(R.P - 7)


def _scalar(tag, i):
    return int.from_bytes(hashlib.shake_256(b"dec-scalar-%s-%d" % (tag, i)).digest(64), "little") % C.L


def _kind(bpp, call):
    """0 if call() returns, else the ProofError kind"""
    try:
        call()
        return OK
    except bpp.ProofError as e:
        return int(e.kind)


# ------------------------------------------------------------------------------------------------- the plain form
def test_plain_form_decodes_every_valid_member(engine):
    one = sb(1)
    for name, b in VALID:
        assert engine.msm_vartime([one], [b]) == b, name
    scalars = [_scalar(b"all", i) for i in range(len(VALID))]
    want = C.multiscalar_mul(scalars, [C.decompress(b) for _, b in VALID]).compress()
    assert engine.msm_vartime([sb(s) for s in scalars], [b for _, b in VALID]) == want


def test_plain_form_refuses_every_other_member(bpp, engine):
    one = sb(1)
    for name, b in INVALID:
        assert _kind(bpp, lambda: engine.msm_vartime([one], [b])) == INVALID_ARGUMENT, (name, R.classify(b))


@pytest.mark.parametrize("n,at", [(65, 64), (65, 63)])
def test_plain_form_bad_point_at_the_wave_tail_and_edge(bpp, engine, n, at):
    """one wavefront decodes 64 points: the only bad one is the single lane of the second wavefront, or the last lane of the first"""
    good = [b for _, b in VALID if b != bytes(32)]
    pts = [good[i % len(good)] for i in range(n)]
    scalars = [_scalar(b"tail", i) for i in range(n)]
    want = C.multiscalar_mul(scalars, [C.decompress(b) for b in pts]).compress()
    assert engine.msm_vartime([sb(s) for s in scalars], pts) == want
    for name, b in NAMED_INVALID:
        bad = list(pts)
        bad[at] = b
        assert _kind(bpp, lambda: engine.msm_vartime([sb(s) for s in scalars], bad)) == INVALID_ARGUMENT, (name, at)
    assert engine.msm_vartime([sb(s) for s in scalars], pts) == want  # and nothing of the refusals stays behind


def test_plain_form_behind_msm_ct(bpp, engine):
    s = _scalar(b"ct", 0)
    other = C.BASEPOINT * 5
    for name, b in R.NAMED:
        pt = C.decompress(b)
        call = lambda: engine.msm_ct([sb(s), sb(3)], [b, other.compress()])  # noqa: E731
        if pt is None:
            assert _kind(bpp, call) == INVALID_ARGUMENT, name
        else:
            assert call() == (pt * s + other * 3).compress(), name


def test_plain_form_behind_precomputation_and_mixed_dynamic_points(bpp, engine):
    s0, s1, s2 = (_scalar(b"mix", i) for i in range(3))
    fixed = C.BASEPOINT * 7
    table = engine.precomputation([fixed.compress()])
    for name, b in R.NAMED:
        pt = C.decompress(b)
        if pt is None:
            assert _kind(bpp, lambda: engine.precomputation([fixed.compress(), b])) == INVALID_ARGUMENT, name
            assert _kind(bpp, lambda: table.vartime_mixed_multiscalar_mul([sb(s0)], [sb(s1)], [b])) == INVALID_ARGUMENT, name
            continue
        pc = engine.precomputation([fixed.compress(), b])  # the member as a static point: the created table must multiply
        assert pc.vartime_mixed_multiscalar_mul([sb(s0), sb(s1)], [sb(s2)], [fixed.compress()]) == \
            (fixed * s0 + pt * s1 + fixed * s2).compress(), name
        pc.close()
        assert table.vartime_mixed_multiscalar_mul([sb(s0)], [sb(s1)], [b]) == (fixed * s0 + pt * s1).compress(), name
    table.close()


def test_plain_form_behind_the_pedersen_bases(bpp, engine):
    """bpp_params_create: the member as H, and as the last of t = 2 G bases.  The identity decodes and is refused as
    validate_and_append_point refuses it (VerificationFailed); a member that does not decode is InvalidArgument"""
    g = [(C.BASEPOINT * 11).compress(), (C.BASEPOINT * 13).compress()]
    h = (C.BASEPOINT * 17).compress()
    for name, b in R.NAMED:
        want = OK if C.decompress(b) is not None else INVALID_ARGUMENT
        if b == bytes(32):
            want = VERIFICATION_FAILED
        for gens in (bpp.PedersenGens(2, b, g), bpp.PedersenGens(2, h, [g[0], b])):
            made = []
            got = _kind(bpp, lambda: made.append(bpp.RangeParameters.init(8, 1, gens, engine=engine)))
            assert got == want, (name, got)
            for p in made:
                assert p.h_base_compressed() == gens.h_base_compressed and p.g_bases_compressed() == gens.g_base_compressed_vec
                v, r = 2**64 - 1, [_scalar(b"ped", 0), _scalar(b"ped", 1)]
                pts = [C.decompress(x) for x in [gens.h_base_compressed] + gens.g_base_compressed_vec]
                assert p.commit(v, [sb(x) for x in r]) == C.multiscalar_mul([v] + r, pts).compress(), name
                p.close()


# ------------------------------------------------------------------------------------------------- the lean form
_CASES = {}


def _case(bpp, engine, count):
    """`count` oracle-made proofs of (n, m, t) = (8, 1, 1): three rounds, nine proof points each"""
    if count not in _CASES:
        _CASES[count] = attach_product(make_oracle_batch(8, [1] * count, 1, seed=b"decode-%d" % count), bpp, engine)
    return _CASES[count]


def _slot_offset(raw, slot, t=1):
    pA = 1 + 32 * t
    rounds = (len(raw) - pA - 160) // 64
    return {"A": pA, "A1": pA + 32, "B": pA + 64, "L_0": pA + 160, "R_last": pA + 160 + 64 * (rounds - 1) + 32}[slot]


def _put(raw, off, member):
    return raw[:off] + member + raw[off + 32:]


# proof point k of a proof in the order k_decompress walks them (the dynamic-slot order without the commitments): A1, B, A, L.., R..
def _point_offset(raw, k, t=1):
    pA = 1 + 32 * t
    rounds = (len(raw) - pA - 160) // 64
    if k < 3:
        return (pA + 32, pA + 64, pA)[k]
    k -= 3
    return pA + 160 + 64 * k if k < rounds else pA + 160 + 64 * (k - rounds) + 32


def _oracle_kind(c, proofs_bytes, statements=None):
    try:
        proofs = [O.RangeProof.from_bytes(b) for b in proofs_bytes]
        O.verify([M.Transcript(c.label) for _ in proofs], statements or c.o_statements_public, proofs, O.VERIFY_ONLY)
        return OK
    except O.ProofError as e:
        return int(e.kind)


def _product_kind(bpp, c, proofs_bytes, statements=None):
    return _kind(bpp, lambda: bpp.RangeProof.verify_batch(c.transcripts(), statements or c.statements_public,
                                                         [bpp.RangeProof.from_bytes(b) for b in proofs_bytes], bpp.VerifyAction.VerifyOnly))


def _rule(member):
    """what test_lean_form_member_at_a_slot establishes against the oracle for a substituted member, at every slot"""
    return VERIFICATION_FAILED if C.decompress(member) is not None else INVALID_ARGUMENT


@pytest.mark.parametrize("slot", ["A", "A1", "B", "L_0", "R_last", "commitment"])
def test_lean_form_member_at_a_slot(bpp, engine, slot):
    """every named member in place of one proof point, or as the statement's commitment (decoded once, at upload), through the item
    call: the oracle's outcome on the same bytes"""
    c = _case(bpp, engine, 1)
    raw = c.o_proofs[0].to_bytes()
    assert _product_kind(bpp, c, [raw]) == OK
    for name, b in R.NAMED:
        if slot == "commitment":
            pt = C.decompress(b)
            mins = c.o_statements_public[0].minimum_value_promises
            want = INVALID_ARGUMENT if pt is None else _oracle_kind(c, [raw], [O.RangeStatement(c.o_params, [pt], mins, None)])
            got = _product_kind(bpp, c, [raw], [bpp.RangeStatement.init(c.params, [b], mins, None)])
        else:
            mutated = _put(raw, _slot_offset(raw, slot), b)
            want = _oracle_kind(c, [mutated])
            got = _product_kind(bpp, c, [mutated])
        assert got == want, (slot, name, R.classify(b), got, want)
        assert want == _rule(b), (slot, name, want)
    assert _product_kind(bpp, c, [raw]) == OK


def test_lean_form_random_members_at_slot_a(bpp, engine):
    """the rule -- InvalidArgument when the member does not decode, VerificationFailed when it does -- is the oracle's for one member
    of every class, and then holds for all 400 random members"""
    c = _case(bpp, engine, 1)
    raw = c.o_proofs[0].to_bytes()
    off = _slot_offset(raw, "A")
    seen = set()
    for name, b in R.CORPUS:
        if R.classify(b) not in seen:
            seen.add(R.classify(b))
            assert _oracle_kind(c, [_put(raw, off, b)]) == _rule(b), (name, R.classify(b))
    assert seen == set(R.CLASSES)
    for name, b in R.RANDOM:
        assert _product_kind(bpp, c, [_put(raw, off, b)]) == _rule(b), (name, R.classify(b))


def test_lean_form_through_the_packed_call_and_a_resident_batch(bpp, engine):
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    c = _case(bpp, engine, 1)
    raw = c.o_proofs[0].to_bytes()
    off = _slot_offset(raw, "A")
    st = c.o_statements_public[0]
    comm = np.frombuffer(st.commitments_compressed[0], dtype=np.uint8).reshape(1, 1, 32)
    mins = np.array([[v if v is not None else 0 for v in st.minimum_value_promises]], dtype=np.uint64)
    pres = np.array([[1 if v is not None else 0 for v in st.minimum_value_promises]], dtype=np.uint8)

    def packed_call(blob):
        inp = packed.PackedInput(np.frombuffer(blob, dtype=np.uint8).reshape(1, -1), comm, mins, pres, None, LABEL)
        return _kind(bpp, lambda: packed.verify_batch(c.params, inp, bpp.VerifyAction.VerifyOnly, 0))
    assert packed_call(raw) == OK
    for name, b in R.NAMED:
        mutated = _put(raw, off, b)
        assert packed_call(mutated) == _rule(b), name
        rb = bpp.ResidentBatch(c.transcripts(), c.statements_public, [bpp.RangeProof.from_bytes(mutated)])
        first = _kind(bpp, lambda: rb.verify(bpp.VerifyAction.VerifyOnly, chunk=0))
        again = _kind(bpp, lambda: rb.verify(bpp.VerifyAction.VerifyOnly, chunk=0))  # the status words are reset between passes
        assert (first, again) == (_rule(b), _rule(b)), name
        clean = bpp.ResidentBatch(c.transcripts(), c.statements_public, c.proofs)  # and nothing leaks into the next batch
        assert clean.verify(bpp.VerifyAction.VerifyOnly, chunk=0) == [None], name
        clean.close()
        rb.close()
    assert packed_call(raw) == OK


# proof point index (the lane of k_decompress, the column of the spill array) -> (proof, point of the proof): 72 points, two
# wavefronts, the second partial; 63 / 64 are the first wavefront's last lane and the second's first, 71 the last point
POSITIONS = [63, 64, 71]


def _position_blobs(c):
    raws = [p.to_bytes() for p in c.o_proofs]
    out = []
    for at in POSITIONS:
        proof, k = divmod(at, 9)
        blobs = list(raws)
        blobs[proof] = _put(raws[proof], _point_offset(raws[proof], k), T_NEGATIVE)
        out.append(blobs)
    # the same numbers as indices into ALL dynamic slots (ten per proof: the commitment first)
    for at in POSITIONS[:2]:
        proof, k = divmod(at, 10)
        blobs = list(raws)
        blobs[proof] = _put(raws[proof], _point_offset(raws[proof], k - 1), T_NEGATIVE)
        out.append(blobs)
    return raws, out


def test_lean_form_bad_point_at_the_wave_edge_and_tail(bpp, engine):
    c = _case(bpp, engine, 8)
    raws, cases = _position_blobs(c)
    assert len(raws) == 8 and all(len(r) == 1 + 32 * 12 for r in raws)
    assert _oracle_kind(c, raws) == OK and _product_kind(bpp, c, raws) == OK
    for blobs in cases:
        want = _oracle_kind(c, blobs)
        assert want == INVALID_ARGUMENT and _product_kind(bpp, c, blobs) == want
        assert _product_kind(bpp, c, raws) == OK


@pytest.mark.parametrize("side", [0, 1])
def test_lean_form_beside_pass1_and_after_it(bpp, engine, opt, side):
    opt("side_decompress", side)
    c = _case(bpp, engine, 1)
    raw = c.o_proofs[0].to_bytes()
    off = _slot_offset(raw, "A")
    for name, b in R.NAMED:
        assert _product_kind(bpp, c, [_put(raw, off, b)]) == _rule(b), (side, name)
    assert _product_kind(bpp, c, [raw]) == OK
    c8 = _case(bpp, engine, 8)
    raws, cases = _position_blobs(c8)
    assert [_product_kind(bpp, c8, blobs) for blobs in cases] == [INVALID_ARGUMENT] * len(cases)
    assert _product_kind(bpp, c8, raws) == OK


@pytest.mark.parametrize("slot", ["A", "commitment"])
def test_lean_form_value_at_the_edges(bpp, engine, slot):
    """the decoded VALUE of the smallest and the largest valid s: the final multiscalar sum of a rejected pass, read back from the
    resident batch, is the oracle's point (a wrong x or y that is still on the curve would be rejected all the same)"""
    c = _case(bpp, engine, 1)
    raw = c.o_proofs[0].to_bytes()
    mins = c.o_statements_public[0].minimum_value_promises
    for name in ("4", "6", "p-3", "20"):
        b = dict(R.NAMED)[name]
        if slot == "A":
            blob, o_sts, sts = _put(raw, _slot_offset(raw, "A"), b), c.o_statements_public, c.statements_public
        else:
            blob = raw
            o_sts = [O.RangeStatement(c.o_params, [C.decompress(b)], mins, None)]
            sts = [bpp.RangeStatement.init(c.params, [b], mins, None)]
        trace = {}
        O.verify([M.Transcript(c.label)], o_sts, [O.RangeProof.from_bytes(blob)], O.VERIFY_ONLY, trace=trace, check=False)
        assert trace["msm_result"] != bytes(32)
        rb = bpp.ResidentBatch(c.transcripts(), sts, [bpp.RangeProof.from_bytes(blob)])
        assert _kind(bpp, lambda: rb.verify(bpp.VerifyAction.VerifyOnly, chunk=0)) == VERIFICATION_FAILED
        assert rb.trace(5) == b"".join(sb(x) for x in trace["dynamic_scalars"]), name
        assert rb.trace(6) == trace["msm_result"], name
        rb.close()


# ------------------------------------------------------------------------------------------------- the lean form without spill
_CHILD = r'''
import importlib, json, sys
sys.path.insert(0, {root!r})
bpp = importlib.import_module("bulletproofs-plus_amd")
job = json.load(open(sys.argv[1]))
eng = bpp.Engine(0)
params = bpp.RangeParameters.init(job["n"], job["m_max"], bpp.create_pedersen_gens_with_extension_degree(job["t"]), engine=eng)
out = []
for call in job["calls"]:
    sts = [bpp.RangeStatement.init(params, [bytes.fromhex(x) for x in cs], mins, None) for cs, mins in call["statements"]]
    trs = [bpp.Transcript.new(bytes.fromhex(job["label"])) for _ in sts]
    try:
        bpp.RangeProof.verify_batch(trs, sts, [bpp.RangeProof.from_bytes(bytes.fromhex(p)) for p in call["proofs"]], bpp.VerifyAction.VerifyOnly)
        out.append(0)
    except bpp.ProofError as e:
        out.append(int(e.kind))
params.close()
eng.close()
print("RESULT " + json.dumps(out))
'''


def test_lean_form_without_the_spill_array(bpp, engine, tmp_path):
    """BPP_DECOMPRESS_SPILL=0 (read once per process): the named members at slot A and the position test in one fresh process"""
    c1, c8 = _case(bpp, engine, 1), _case(bpp, engine, 8)
    raw = c1.o_proofs[0].to_bytes()
    off = _slot_offset(raw, "A")

    def call(c, blobs):
        return {"proofs": [b.hex() for b in blobs],
                "statements": [([x.hex() for x in s.commitments_compressed], s.minimum_value_promises) for s in c.o_statements_public]}
    calls, want = [call(c1, [raw])], [OK]
    for name, b in R.NAMED:
        calls.append(call(c1, [_put(raw, off, b)]))
        want.append(_rule(b))
    raws, cases = _position_blobs(c8)
    for blobs in [raws] + cases + [raws]:
        calls.append(call(c8, blobs))
    want += [OK] + [INVALID_ARGUMENT] * len(cases) + [OK]
    job = tmp_path / "job.json"
    job.write_text(json.dumps({"n": 8, "m_max": 1, "t": 1, "label": LABEL.hex(), "calls": calls}))
    script = tmp_path / "nospill_child.py"
    script.write_text(_CHILD.format(root=ROOT))
    r = subprocess.run([sys.executable, str(script), str(job)], env=dict(os.environ, BPP_DECOMPRESS_SPILL="0"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads([x for x in r.stdout.splitlines() if x.startswith("RESULT ")][0][7:])
    assert got == want, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
