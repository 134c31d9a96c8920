"""GPU tests of the constant-time multiscalar multiplication of seam B1 (bpp_msm_ct, bpp_msm_ct_batched; csrc/ct.h: k_ct_straus<K> +
k_ct_straus_sum): every result is held against the oracle's MSM and against the bytes of the variable-time entry point for the same
input, in both kernel forms ("msm_ct_k" = 1 and = 2).

Term counts sit on both forms' chunk boundaries (16 and 32 terms), one short and one over, and span several chunks per group (64,
65, 100); the ragged batch has empty groups, a one-term group, a group on the boundary and one over it.  The commitment shape is
held against bpp_pedersen_commit, an independent device path (k_ct_fixed)."""
import hashlib

import pytest

from oracle.pyref import curve as C
from tests.helpers import sb

pytestmark = pytest.mark.gpu

L = C.L
IDENT = bytes(32)
FORMS = [1, 2]
_CACHE = {}


def _h(tag, i, n=32):
    return hashlib.shake_256(b"%s-%d" % (tag, i)).digest(n)


def edge_scalars():
    """0, 1, l - 1, 2^252, 2^252 - 1, every digit 8 (the longest carry chain of the recoding), every digit 7"""
    return [0, 1, L - 1, 2**252, 2**252 - 1, int("8" * 63, 16), int("7" * 63, 16)]


def _inputs(n):
    """n (scalar, point) terms, the same for every test (prefixes of one list): random points with the identity encoding (i = 3 mod
    11) and a repeated point (i = 7 mod 11) mixed in; random scalars with the edge scalars at i = 0, 5, 10, ..  The references are
    computed once per term count."""
    if "all" not in _CACHE:
        pts, scalars = [], []
        edge = edge_scalars()
        for i in range(140):
            if i % 11 == 3:
                pts.append(C.Point.identity())
            elif i % 11 == 7:
                pts.append(pts[i - 2])
            else:
                pts.append(C.from_uniform_bytes(_h(b"ct-p", i, 64)))
            scalars.append(edge[(i // 5) % len(edge)] if i % 5 == 0 else int.from_bytes(_h(b"ct-s", i), "little") % L)
        _CACHE["all"] = (scalars, pts, [sb(s) for s in scalars], [p.compress() for p in pts])
    s, p, s32, p32 = _CACHE["all"]
    return s[:n], p[:n], s32[:n], p32[:n]


def _want(lo, hi):
    key = ("want", lo, hi)
    if key not in _CACHE:
        s, p, _, _ = _inputs(hi)
        prod = _CACHE.setdefault("prod", {})  # every term's product once, whatever ranges ask for it
        acc = C.Point.identity()
        for i in range(lo, hi):
            if i not in prod:
                prod[i] = C.multiscalar_mul([s[i]], [p[i]])
            acc = acc + prod[i]
        _CACHE[key] = acc.compress() if hi > lo else IDENT
    return _CACHE[key]


@pytest.mark.parametrize("K", FORMS)
@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 31, 32, 33, 64, 65, 100])
def test_single_group_parity(bpp, engine, opt, K, n):
    _, _, s32, p32 = _inputs(n)
    opt("msm_ct_k", K)
    got = engine.msm_ct(s32, p32)
    assert got == _want(0, n)
    assert got == engine.msm_vartime(s32, p32)


@pytest.mark.parametrize("K", FORMS)
def test_edge_scalars_and_points(bpp, engine, opt, K):
    opt("msm_ct_k", K)
    p = C.from_uniform_bytes(_h(b"ct-e", 0, 64))
    pc, nc = p.compress(), (-p).compress()
    assert engine.msm_ct([], []) == IDENT                                  # no terms: nothing is launched
    for k in edge_scalars() + [int.from_bytes(_h(b"ct-e", 1), "little") % L]:
        assert engine.msm_ct([sb(k)], [pc]) == (p * k).compress(), hex(k)
        assert engine.msm_ct([sb(k)], [IDENT]) == IDENT                    # the identity encoding under every scalar
        assert engine.msm_ct([sb(k), sb(k)], [pc, nc]) == IDENT            # P and -P under equal scalars
        assert engine.msm_ct([sb(k), sb(k)], [pc, pc]) == (p * (2 * k % L)).compress()  # a repeated point


@pytest.mark.parametrize("K", FORMS)
def test_batched_parity(bpp, engine, opt, K):
    sizes = [0, 1, 16, 17, 0, 40, 2, 0]
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    _, _, s32, p32 = _inputs(off[-1])
    opt("msm_ct_k", K)
    got = engine.msm_ct_batched(s32, p32, off)
    assert got == [_want(a, b) for a, b in zip(off, off[1:])]
    assert got == engine.msm_vartime_batched(s32, p32, off)
    assert [g for g, s in zip(got, sizes) if s == 0] == [IDENT] * 3       # empty groups give 32 zero bytes


@pytest.mark.parametrize("K", FORMS)
@pytest.mark.parametrize("t", [1, 6])
def test_commitment_shape(bpp, engine, opt, K, t):
    """1 + t terms per group over a parameter set's exported H and G_0 .. G_{t-1} == bpp_pedersen_commit (k_ct_fixed)"""
    params = bpp.RangeParameters.init(8, 1, bpp.create_pedersen_gens_with_extension_degree(t), engine=engine)
    try:
        values = [0, 1, 2**64 - 1, 0x0123456789abcdef, 2**63]
        blind = [[sb(int.from_bytes(_h(b"ct-b%d" % t, 8 * j + k), "little") % L) for k in range(t)] for j in range(len(values))]
        blind[0] = [sb(0)] * t  # value 0 under blinding factors 0: the neutral element
        blind[1][0] = sb(L - 1)
        want = params.commit_many(values, blind)
        bases = [params.h_base_compressed()] + params.g_bases_compressed()
        scalars, points = [], []
        for v, b in zip(values, blind):
            scalars += [sb(v)] + b
            points += bases
        opt("msm_ct_k", K)
        got = engine.msm_ct_batched(scalars, points, [(1 + t) * j for j in range(len(values) + 1)])
        assert got == want
        assert got[0] == IDENT
    finally:
        params.close()


def _expect_invalid(bpp, call):
    with pytest.raises(bpp.ProofError) as e:
        call()
    assert e.value.kind == bpp.ProofErrorKind.InvalidArgument


@pytest.mark.parametrize("K", FORMS)
def test_errors_and_hygiene(bpp, K):
    """the scalar l first or last, a point that does not decode: InvalidArgument, nothing secret left behind, and the next call on the
    same context is right.  A context of its own: `examined` is 0 before a context's first call."""
    eng = bpp.Engine(0)
    try:
        eng.set_option("msm_ct_k", K)
        assert eng.msm_ct_secret_bytes() == (0, 0)
        n = 33
        _, _, s32, p32 = _inputs(n)
        off = [0, 16, 33]
        ell = L.to_bytes(32, "little")
        bad_point = b"\x01" + bytes(31)  # a negative s: no canonical encoding
        failing = [
            lambda: eng.msm_ct([ell] + s32[1:], p32),
            lambda: eng.msm_ct(s32[:-1] + [ell], p32),
            lambda: eng.msm_ct_batched(s32[:-1] + [ell], p32, off),
            lambda: eng.msm_ct(s32, p32[:20] + [bad_point] + p32[21:]),
            lambda: eng.msm_ct_batched(s32, [bad_point] + p32[1:], off),
        ]
        for k, call in enumerate(failing):
            _expect_invalid(bpp, call)
            seen, nonzero = eng.msm_ct_secret_bytes()
            assert nonzero == 0, (k, nonzero)
            assert eng.msm_ct(s32, p32) == _want(0, n)
            seen, nonzero = eng.msm_ct_secret_bytes()
            assert seen >= 32 * n and nonzero == 0, (k, seen, nonzero)
        assert eng.msm_ct_batched(s32, p32, off) == [_want(0, 16), _want(16, 33)]
        seen, nonzero = eng.msm_ct_secret_bytes()
        assert seen > 0 and nonzero == 0
    finally:
        eng.close()


@pytest.mark.parametrize("K", FORMS)
def test_independent_of_the_bucket_method_options(bpp, engine, opt, K):
    n = 40
    _, _, s32, p32 = _inputs(n)
    opt("msm_ct_k", K)
    opt("msm_plain", 1)
    assert engine.msm_ct(s32, p32) == _want(0, n)
    plan = engine.msm_last_plan()
    assert plan["ct"] and plan["G"] == 1 and plan["terms"] == n and plan["form"] == 64
    assert [plan[k] for k in ("c", "K", "K_wide", "nb", "dig_cap")] == [0] * 5
    off = [0, 3, 3, 40]
    assert engine.msm_ct_batched(s32, p32, off) == [_want(0, 3), IDENT, _want(3, 40)]
    plan = engine.msm_last_plan()
    assert plan["ct"] and plan["G"] == 3 and plan["terms"] == n
    assert engine.msm_vartime(s32, p32) == _want(0, n)
    plan = engine.msm_last_plan()
    assert plan["plain"] and not plan["ct"]
    opt("msm_plain", 0)
    assert engine.msm_vartime(s32, p32) == _want(0, n)
    assert not engine.msm_last_plan()["ct"] and not engine.msm_last_plan()["plain"]


def test_form_option_values(bpp, engine, opt):
    """0 and -1 both mean the engine's rule; whatever form it takes, the bytes are the same"""
    for n in (16, 17):
        _, _, s32, p32 = _inputs(n)
        for v in (0, -1, 1, 2):
            opt("msm_ct_k", v)
            assert engine.msm_ct(s32, p32) == _want(0, n)
