"""GPU tests of the bucket MSM (csrc/msm.h) behind the B1 calls -- msm_vartime, msm_vartime_batched, the precomputation's mixed
call -- under STRUCTURED scalars, in every kernel form the engine can take.

Every other oracle test of the bucket method draws its scalars from a hash: all buckets about equally full, no window empty, no
bucket with the same point twice or a sum that passes through the identity.  A B1 caller passes whatever it holds.  The families
of tests/helpers.py (msm_structured_cases; tests/test_host_arith.py checks that they are what they claim to be) reach what only
such inputs reach: size classes clamped to 255, terms past the prelude's digit cache, list lengths 1..9 of the two software
pipelines, the first-term start of an accumulator, empty buckets and empty windows, doublings and cancellations inside a list.

Oracle: oracle.pyref.curve.multiscalar_mul over the scalars folded per distinct point.  The 32 output bytes are compared exactly:
there is no tolerance in this file.  After every call the form the call TOOK (Engine.msm_last_plan) is held against the form the
row is there for, so a change of choose_window or of the quad rule cannot quietly fold two rows into one.

Measured on an MI355X: the 25 000-term ids take 0.8 s (quad forms) to 1.2 s (one lane per bucket) each, oracle included, every
other id under 0.5 s."""
import pytest

from oracle.pyref import curve as C
from tests import helpers as H

pytestmark = pytest.mark.gpu

IDENT = bytes(32)
_SB, _ENC, _CASES = {}, [], {}


def _sb(x):
    b = _SB.get(x)
    if b is None:
        b = _SB[x] = H.sb(x)
    return b


def _enc():
    if not _ENC:
        _ENC.extend(p.compress() for p in H.msm_bases())
        assert _ENC[H.MSM_IDENT] == IDENT and len(set(_ENC)) == 15
    return _ENC


def _cases(n, c):
    """the families at n terms; everything but the chains is the same for every c and built (and its oracle result computed) once"""
    if n not in _CASES:
        _CASES[n] = [x for x in H.msm_structured_cases(n, 4) if not x.name.startswith("chains-")]
    if (n, c) not in _CASES:
        _CASES[n, c] = H.msm_chains(n, c)
    return _CASES[n] + [_CASES[n, c]]


def _want(case):
    """the oracle's result, computed once per case object (the cases above are shared by all rows)"""
    if not hasattr(case, "want"):
        case.want = case.expected()
    return case.want


def _args(case):
    enc = _enc()
    return [_sb(s) for s in case.scalars], [enc[p] for p in case.pidx]


SMALL_GROUP_TERMS = 9000  # csrc/msm.h: BPP_SORT_SMALL_GROUP_TERMS, up to which a lane-form call takes the 256-lane prelude


def _check_plan(plan, case, c, terms, G, quad, reduce, final_quad=True, max_group=None):
    max_group = terms if max_group is None else max_group
    want = {"plain": False, "c": c, "nb": 1 << (c - 1), "K": -(-253 // c), "G": G, "terms": terms, "quad": quad, "reduce": reduce,
            "final_quad": final_quad, "narrow_prelude": not quad and max_group <= SMALL_GROUP_TERMS}
    if G == 1:  # the digits of the first dig_cap terms are cached in LDS: all of them, or as many as fit beside 2 x nb counters
        want["dig_cap"] = min(terms, H.MSM_DIG_CAPS.get(c, terms))
    got = {k: plan[k] for k in want}
    assert got == want, (case, got, want)
    assert plan["K_wide"] * c + (plan["K"] - plan["K_wide"]) * (c - 1) == 253


# (n, options, c, quad, reduction, final_quad): the form the row is there for
def _rows():
    rows = []
    for q in (1, 0):
        rows.append((100, {"msm_c_bias": 0, "msm_quad": q}, 4, bool(q), "rc_quad" if q else "rc2", True))
    for bias in range(7):
        rows.append((300, {"msm_c_bias": bias, "msm_quad": 1}, 5 + bias, True, "rc_quad", True))
    for bias in range(7):
        rows.append((300, {"msm_c_bias": bias, "msm_quad": 0}, 5 + bias, False, "rc2" if 5 + bias <= 9 else "rc", True))
    for bias in (0, 4):
        rows.append((300, {"msm_c_bias": bias, "msm_quad": 0, "msm_rc2": 0}, 5 + bias, False, "rc", True))
    for bias in (0, 6):
        for fq in (0, 1):
            rows.append((300, {"msm_c_bias": bias, "msm_final_quad": fq}, 5 + bias, True, "rc_quad", bool(fq)))
    rows.append((25000, {}, 11, True, "rc_quad", True))
    for add in (0, 1, 2):
        for q in (0, 1):
            rows.append((25000, {"msm_c_max": 14, "msm_c_add": add, "msm_quad": q}, 12 + add, bool(q), "bitsum", True))
    return rows


def _row_id(row):
    return "n%d-%s" % (row[0], "-".join("%s%d" % (k[4:], v) for k, v in row[1].items()) or "default")


@pytest.mark.parametrize("row", _rows(), ids=_row_id)
def test_structured_scalars_in_every_form(bpp, engine, opt, row):
    n, options, c, quad, reduce, final_quad = row
    for k, v in options.items():
        opt(k, v)
    opt("msm_plain", 0)
    for case in _cases(n, c):
        got = engine.msm_vartime(*_args(case))
        _check_plan(engine.msm_last_plan(), case.name, c, n, 1, quad, reduce, final_quad)
        assert got == _want(case), (case.name, got.hex())


@pytest.mark.parametrize("n", [100, 300, 25000])
def test_structured_scalars_plain_kernels(bpp, engine, opt, n):
    """the verifier's recheck path (msm_plain.h) sees the same inputs and must give the same bytes"""
    opt("msm_plain", 1)
    for case in _cases(n, 11 if n > 20000 else 5):
        got = engine.msm_vartime(*_args(case))
        plan = engine.msm_last_plan()
        assert plan["plain"] and plan["form"] == 32 and plan["terms"] == n and plan["G"] == 1, (case.name, plan)
        assert got == _want(case), (case.name, got.hex())


# ---- one batched call: 27 groups (not a multiple of 8: the tail of the XCD mapping g = xcd + 8 (j / K)), sizes on both sides of a
# wavefront and of the class clamp, a different family in every group
GROUP_SIZES = [0, 1, 63, 64, 65, 254, 255, 256, 257, 300]
_S = H.MSM_CONSTANTS[0][1]
GROUP_FAMILIES = [  # group g has GROUP_SIZES[g % 10] terms; the empty groups 0, 10 and 20 are the empty sum whatever builds them
    # 0, 1, 63, 64, 65 terms, then the four constants at 254, 255, 256 and 257 terms, unpadded, then 300
    lambda n: H.msm_zero(n), lambda n: H.msm_sparse(n, 0), lambda n: H.msm_cancel(n, _S), lambda n: H.msm_cancel3(n, _S),
    lambda n: H.msm_same_point(n, _S), lambda n: H.msm_constant(n, _S), lambda n: H.msm_constant(n, 1),
    lambda n: H.msm_constant(n, C.L - 1), lambda n: H.msm_constant(n, 1 << 252), lambda n: H.msm_identity_terms(n, "first"),
    lambda n: H.msm_zero(n), lambda n: H.msm_identity_terms(n, "alone"), lambda n: H.msm_identity_terms(n, "all"),
    lambda n: H.msm_small(n, 16), lambda n: H.msm_small(n, 64), lambda n: H.msm_sparse(n, n - 1), lambda n: H.msm_ramp(n),
    lambda n: H.msm_ramp(n, 120), lambda n: H.msm_chains(n, 8), lambda n: H.msm_skew(n),
    lambda n: H.msm_zero(n), lambda n: H.msm_prefix(n, 1, _S, "pipeline"), lambda n: H.msm_prefix(n, 9, _S, "pipeline"),
    lambda n: H.msm_cancel(n, _S, n - 1), lambda n: H.msm_identity_terms(n, "middle"), lambda n: H.msm_top(n),
    lambda n: H.msm_prefix(n, 254, _S, "clamp"),
]


@pytest.mark.parametrize("quad", [-1, 1])
def test_structured_scalars_batched_groups(bpp, engine, opt, quad):
    assert len(GROUP_FAMILIES) == 27
    sizes = [GROUP_SIZES[g % len(GROUP_SIZES)] for g in range(27)]
    groups = [GROUP_FAMILIES[g](n) if n else None for g, n in enumerate(sizes)]
    off, scalars, points = [0], [], []
    for g in groups:
        if g is not None:
            s, p = _args(g)
            scalars += s
            points += p
        off.append(len(scalars))
    opt("msm_plain", 0)
    opt("msm_quad", quad)
    got = engine.msm_vartime_batched(scalars, points, off)
    # the engine's own rule: c = 5 + 3 = 8, 27 x 32 x 128 = 110 592 buckets > 100 000 -> one lane per bucket, 256-lane prelude, rc2
    forced = quad == 1
    _check_plan(engine.msm_last_plan(), "batched", 8, off[-1], 27, forced, "rc_quad" if forced else "rc2", max_group=max(sizes))
    assert (engine.msm_last_plan()["K"], engine.msm_last_plan()["nb"]) == (32, 128)
    want = [_want(g) if g is not None else IDENT for g in groups]
    for g in range(27):  # every group against ITS oracle result: nothing leaks across a group boundary
        assert got[g] == want[g], (g, sizes[g], groups[g].name if groups[g] else None, got[g].hex())
    opt("msm_plain", 1)
    assert engine.msm_vartime_batched(scalars, points, off) == want
    assert engine.msm_last_plan()["plain"]


@pytest.mark.parametrize("quad", [0, 1])
def test_structured_scalars_mixed(bpp, engine, opt, quad):
    """70 precomputed points (tab_a), 66 static scalars from the constant, small and sparse families; 20 dynamic terms (tab_b) from
    the cancel and top families"""
    enc, bases = _enc(), H.msm_bases()
    static_idx = [i % 7 for i in range(70)]
    pre = engine.precomputation([enc[i] for i in static_idx])
    static = [_S] * 22 + [H.msm_hashed(b"mixed-small", i, 16 if i & 1 else 64) for i in range(22)] + [0] * 21 + [H.msm_hashed(b"mixed-sparse", 0)]
    dyn_idx = [(3, H.MSM_NEG + 3)[i & 1] for i in range(10)] + [i % 7 for i in range(10)]
    dyn = [_S] * 10 + [H.MSM_TOP[i % 5] for i in range(10)]
    want = H.MsmCase("mixed", static + dyn, static_idx[:66] + dyn_idx, bases).expected()
    try:
        opt("msm_quad", quad)
        for plain in (0, 1):
            opt("msm_plain", plain)
            got = pre.vartime_mixed_multiscalar_mul([_sb(s) for s in static], [_sb(s) for s in dyn], [enc[i] for i in dyn_idx])
            if plain:
                assert engine.msm_last_plan()["plain"]
            else:  # 86 terms: c = 4 + 3
                _check_plan(engine.msm_last_plan(), "mixed", 7, 86, 1, bool(quad), "rc_quad" if quad else "rc2")
            assert got == want, (plain, got.hex())
    finally:
        pre.close()


def test_entry_checks_at_the_edges_of_a_launch(bpp, engine, opt):
    """a point that does not decode in the last lane of the first wavefront, the first of the second, and the call's last term;
    a scalar that is not canonical in the last position"""
    case = _cases(25000, 11)[-1]
    scalars, points = _args(case)
    for at in (63, 64, 24999):
        bad = list(points)
        bad[at] = b"\x01" + bytes(31)
        with pytest.raises(bpp.ProofError) as e:
            engine.msm_vartime(scalars, bad)
        assert e.value.kind == bpp.ProofErrorKind.InvalidArgument, at
    bad = list(scalars)
    bad[-1] = C.L.to_bytes(32, "little")
    with pytest.raises(bpp.ProofError) as e:
        engine.msm_vartime(bad, points)
    assert e.value.kind == bpp.ProofErrorKind.InvalidArgument
    assert engine.msm_vartime(scalars, points) == _want(case)  # and the context still serves the next call
