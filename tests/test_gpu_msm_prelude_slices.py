"""GPU tests of the sliced prelude of the bucket MSM (csrc/msm.h: k_msm_slice_hist, k_msm_slice_scan, k_msm_slice_scatter), forced at
small sizes through the option "msm_prelude_slices" -- by rule it serves groups of 200 000 terms and more (the joint final check of
a large call), which no test of the suite sends.

bpp_msm_vartime and bpp_msm_vartime_batched with S = 2, 3, 7 slices over 1, 2, 63, 64, 65 and 300 terms (S > n: empty slices; 63 /
64 / 65: on both sides of a wavefront of a slice) and the structured scalar families of tests/helpers.py (all zero, all l - 1,
cancelling pairs, one bucket, ramps, ...), in every reduction form the way tests/test_gpu_msm_structured.py forces them.  Oracle:
each case's expected() (oracle.pyref.curve.multiscalar_mul), 32 bytes compared exactly.  After every call bpp_msm_last_plan must
show the sliced form with the forced S."""
import importlib

import numpy as np
import pytest

from tests import helpers as H
from tests.helpers import LABEL

pytestmark = pytest.mark.gpu

IDENT = bytes(32)
SIZES = [1, 2, 63, 64, 65, 300]
SLICES = [2, 3, 7]
_SB, _ENC, _CASES = {}, [], {}


def _sb(x):
    b = _SB.get(x)
    if b is None:
        b = _SB[x] = H.sb(x)
    return b


def _enc():
    if not _ENC:
        _ENC.extend(p.compress() for p in H.msm_bases())
    return _ENC


def _cases(n):
    """the families at n terms, built (and their oracle results computed) once for all rows"""
    if n not in _CASES:
        _CASES[n] = H.msm_structured_cases(n, 5)
        for x in _CASES[n]:
            x.want = x.expected()
    return _CASES[n]


def _args(case):
    enc = _enc()
    return [_sb(s) for s in case.scalars], [enc[p] for p in case.pidx]


def _check_plan(plan, S, G, terms, quad, reduce, what):
    want = {"sliced_prelude": True, "slices": S, "dig_cap": 0, "plain": False, "G": G, "terms": terms, "quad": quad, "reduce": reduce}
    got = {k: plan[k] for k in want}
    assert got == want, (what, got, want)
    assert plan["form"] & 128 and (plan["form"] >> 8) & 0xff == S


# (options, quad, reduction): each reduction form a small call can take
FORMS = [
    ({"msm_c_bias": 0, "msm_quad": 1}, True, "rc_quad"),
    ({"msm_quad": 0}, False, "rc2"),
    ({"msm_c_bias": 6, "msm_quad": 0, "msm_rc2": 0}, False, "rc"),
    ({"msm_c_bias": 6, "msm_quad": 1, "msm_final_quad": 0}, True, "rc_quad"),
]


@pytest.mark.parametrize("S", SLICES)
@pytest.mark.parametrize("form", range(len(FORMS)), ids=["rc_quad-c0", "rc2", "rc", "rc_quad-final0"])
def test_sliced_prelude_under_structured_scalars(bpp, engine, opt, S, form):
    options, quad, reduce = FORMS[form]
    for k, v in options.items():
        opt(k, v)
    opt("msm_plain", 0)
    opt("msm_prelude_slices", S)
    for n in SIZES:
        for case in _cases(n):
            got = engine.msm_vartime(*_args(case))
            _check_plan(engine.msm_last_plan(), S, 1, n, quad, reduce, case.name)
            assert got == case.want, (case.name, got.hex())
    # and the same call without the option takes the one-workgroup form and gives the same bytes
    opt("msm_prelude_slices", 0)
    case = _cases(300)[0]
    assert engine.msm_vartime(*_args(case)) == case.want
    plan = engine.msm_last_plan()
    assert not plan["sliced_prelude"] and plan["slices"] == 0 and plan["dig_cap"] == 300


@pytest.mark.parametrize("S", SLICES)
def test_bitsum_reduction_at_twelve_bits(bpp, engine, opt, S):
    """windows above 11 bits (the bit-plane reduction) need a call past the small-call rule: 25 000 terms, c = 12, slices of
    12 500, 8 334 and 3 572 terms over the 256-lane workgroups"""
    n = 25000
    opt("msm_c_max", 14)
    opt("msm_quad", 0)
    opt("msm_plain", 0)
    opt("msm_prelude_slices", S)
    if ("big", n) not in _CASES:
        s = H.MSM_CONSTANTS[0][1]
        _CASES["big", n] = [H.msm_skew(n), H.msm_ramp(n), H.msm_top(n), H.msm_cancel(n, s, n - 1), H.msm_prefix(n, 257, s, "clamp")]
        for x in _CASES["big", n]:
            x.want = x.expected()
    for case in _CASES["big", n]:
        got = engine.msm_vartime(*_args(case))
        plan = engine.msm_last_plan()
        _check_plan(plan, S, 1, n, False, "bitsum", case.name)
        assert plan["c"] == 12 and not plan["narrow_prelude"]
        assert got == case.want, (case.name, got.hex())


@pytest.mark.parametrize("S", SLICES)
@pytest.mark.parametrize("quad", [0, 1])
def test_three_groups_of_unequal_size(bpp, engine, opt, S, quad):
    s = H.MSM_CONSTANTS[0][1]
    groups = [H.msm_skew(65), H.msm_sparse(2, 1), H.msm_cancel(300, s, 299)]
    off, scalars, points = [0], [], []
    for g in groups:
        a, b = _args(g)
        scalars += a
        points += b
        off.append(len(scalars))
    opt("msm_plain", 0)
    opt("msm_quad", quad)
    opt("msm_prelude_slices", S)
    got = engine.msm_vartime_batched(scalars, points, off)
    _check_plan(engine.msm_last_plan(), S, 3, 367, bool(quad), "rc_quad" if quad else "rc2", "batched")
    for g, case in enumerate(groups):
        assert got[g] == case.expected(), (g, case.name, got[g].hex())


def test_joint_final_check_through_the_sliced_prelude(bpp, engine, opt):
    """one verifier call of 5 groups x 3 proofs with "verify_joint" = 1 and the slices forced"""
    import bench
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    params = bpp.RangeParameters.init(64, 1, bpp.create_pedersen_gens_with_extension_degree(1), engine=engine)
    try:
        d = bench.make_inputs(np, packed, params, 15, seed=20261020)
        rb = packed.ResidentBatch(params, d["proofs"], d["commitments"], d["min_values"], d["min_present"], None, LABEL)
        try:
            opt("verify_joint", 1)
            opt("msm_prelude_slices", 3)
            s0 = engine.verify_joint_stats()
            res = packed.verify_groups(rb, [0, 3, 6, 9, 12, 15])
            assert all(r["code"] == 0 and r["tier"] == 0 for r in res), res
            assert rb.trace(8) == IDENT
            s1 = engine.verify_joint_stats()
            assert (s1["calls"] - s0["calls"], s1["accepted"] - s0["accepted"], s1["fallbacks"] - s0["fallbacks"]) == (1, 1, 0)
            plan = engine.msm_last_plan()
            assert plan["G"] == 1 and plan["sliced_prelude"] and plan["slices"] == 3 and plan["terms"] == 2 * (130 + 15 * 16), plan
        finally:
            rb.close()
    finally:
        params.close()
