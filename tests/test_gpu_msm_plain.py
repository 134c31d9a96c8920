"""GPU tests of the plain multiscalar multiplication (csrc/msm_plain.h: k_msm_plain + k_msm_plain_sum, option "msm_plain" = 1):
one lane per term, left-to-right double-and-add, a tree through LDS per wavefront, the partials added in index order.  It shares
nothing with the bucket method but the field and point arithmetic, so every result is held against the oracle's MSM AND against
what the bucket method ("msm_plain" = 0) gives for the same input.

Term counts sit on both sides of a wavefront (63, 64, 65) and span several partials per group (1000 = 16 wavefronts); the ragged
batch has groups of 1, 64 and 65 terms and an empty one."""
import hashlib

import pytest

from oracle.pyref import curve as C
from tests.helpers import sb

pytestmark = pytest.mark.gpu

IDENT = bytes(32)
_CACHE = {}


def _h(tag, i, n=32):
    return hashlib.shake_256(b"%s-%d" % (tag, i)).digest(n)


def _inputs(n):
    """n (scalar, point) terms: 40 distinct points repeated, the first scalars the edge values 0, 1, l - 1, 2^252, 2^128"""
    if "pts" not in _CACHE:
        _CACHE["pts"] = [C.from_uniform_bytes(_h(b"plain-p", i, 64)) for i in range(40)]
    base = _CACHE["pts"]
    pts = [base[i % len(base)] for i in range(n)]
    scalars = [int.from_bytes(_h(b"plain-s", i), "little") % C.L for i in range(n)]
    for i, v in zip(range(n), [0, 1, C.L - 1, 2**252, 2**128]):
        scalars[i] = v
    return scalars, pts


def _both(engine, opt, call):
    """call() under the bucket method and under the plain kernels"""
    opt("msm_plain", 0)
    bucket = call()
    opt("msm_plain", 1)
    return bucket, call()


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000])
def test_plain_msm_matches_oracle_and_bucket_method(bpp, engine, opt, n):
    scalars, pts = _inputs(n)
    bucket, plain = _both(engine, opt, lambda: engine.msm_vartime([sb(s) for s in scalars], [p.compress() for p in pts]))
    assert plain == C.multiscalar_mul(scalars, pts).compress()
    assert plain == bucket


def test_plain_msm_edge_scalars_and_points(bpp, engine, opt):
    b = C.BASEPOINT.compress()
    p = C.from_uniform_bytes(_h(b"plain-e", 0, 64))
    cases = [
        ([], []),                                # the empty sum
        ([0], [b]),                              # scalar 0
        ([1], [p.compress()]),                   # scalar 1: the point itself
        ([C.L - 1], [p.compress()]),             # l - 1: the point's negative
        ([7], [IDENT]),                          # the identity point
        ([5, C.L - 5], [b, b]),                  # P and -P cancel (as scalars)
        ([1, 1], [p.compress(), (-p).compress()]),  # P and -P cancel (as points)
        ([0, 0, 0], [b, p.compress(), IDENT]),
    ]
    want = [IDENT, IDENT, p.compress(), (-p).compress(), IDENT, IDENT, IDENT, IDENT]
    for (s, pts), w in zip(cases, want):
        bucket, plain = _both(engine, opt, lambda: engine.msm_vartime([sb(x) for x in s], list(pts)))
        assert plain == w, (s, plain.hex())
        assert plain == bucket
    # the entry checks are the bucket method's: a point that does not decode, a scalar that is not canonical
    opt("msm_plain", 1)
    with pytest.raises(bpp.ProofError) as e:
        engine.msm_vartime([sb(1)], [b"\x01" + bytes(31)])
    assert e.value.kind == bpp.ProofErrorKind.InvalidArgument
    with pytest.raises(bpp.ProofError):
        engine.msm_vartime([C.L.to_bytes(32, "little")], [b])


def test_plain_msm_batched_ragged_groups(bpp, engine, opt):
    sizes = [1, 64, 65, 0, 3, 130, 63]
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    scalars, pts = _inputs(off[-1])
    scalars[70] = 0  # (a zero inside a group as well)
    call = lambda: engine.msm_vartime_batched([sb(s) for s in scalars], [p.compress() for p in pts], off)
    bucket, plain = _both(engine, opt, call)
    want = [C.multiscalar_mul(scalars[a:b], pts[a:b]).compress() if b > a else IDENT for a, b in zip(off, off[1:])]
    assert plain == want
    assert plain == bucket


def test_plain_msm_mixed(bpp, engine, opt):
    scalars, pts = _inputs(90)
    pre = engine.precomputation([p.compress() for p in pts[:70]])
    # 66 static scalars (more than one wavefront of table-A terms, fewer than the table holds) and 20 dynamic terms
    call = lambda: pre.vartime_mixed_multiscalar_mul([sb(s) for s in scalars[:66]], [sb(s) for s in scalars[70:]],
                                                     [p.compress() for p in pts[70:]])
    bucket, plain = _both(engine, opt, call)
    pre.close()
    assert plain == C.multiscalar_mul(scalars[:66] + scalars[70:], pts[:66] + pts[70:]).compress()
    assert plain == bucket


def test_msm_plain_off_values(bpp, engine, opt):
    """0 and -1 both mean off: the call is the bucket method's"""
    scalars, pts = _inputs(5)
    want = C.multiscalar_mul(scalars, pts).compress()
    for v in (0, -1):
        opt("msm_plain", v)
        assert engine.msm_vartime([sb(s) for s in scalars], [p.compress() for p in pts]) == want
