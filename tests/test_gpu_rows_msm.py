"""GPU tests of the constant-time sums and the scalar operation over device rows (bpp_rows_msm_enqueue, bpp_rows_scalar_enqueue;
packed.rows_msm, packed.rows_scalar_muladd; csrc/rows_msm.h).

The reference of every sum is engine.msm_ct_batched on host copies of the rows with group_off = [0, K, 2K, ..] -- k_ct_straus, the
independent kernel path -- and, for a subset, the oracle's multiscalar_mul; the scalar operation is held to Python integers mod l.
The references are computed once per K and shared.  Row counts sit at the rows-per-workgroup boundaries of every padded K (16 / Kp =
16, 8, 4, 2, 1 rows), one below and one over."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from oracle.pyref import curve as C
from tests import transcript_rng_cases as TC
from tests.helpers import sb

pytestmark = pytest.mark.gpu

L = C.L
IDENT = bytes(32)
KS = (1, 2, 3, 4, 5, 8, 9, 16)
NS = (1, 2, 7, 8, 9, 16, 17, 33)
NMAX = max(NS)
WRITTEN, SCALAR, POINT = 1, 2, 4
BAD_POINT = b"\x01" + bytes(31)  # a negative s: no canonical encoding
_CACHE = {}


@pytest.fixture(scope="module")
def packed():
    return importlib.import_module("bulletproofs-plus_amd.packed")


@pytest.fixture(autouse=True)
def no_host_waits(engine, packed):
    yield
    assert packed.rows_stats(engine)["host_waits"] == 0


def _h(tag, i, n=32):
    import hashlib
    return hashlib.shake_256(b"%s-%d" % (tag, i)).digest(n)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(rows):
    """rows of byte strings of one length -> uint8 [n, len]"""
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), -1).copy()


def _pool():
    """48 points and their negatives, encoded once"""
    if "pool" not in _CACHE:
        pts = [C.from_uniform_bytes(_h(b"rows-p", i, 64)) for i in range(48)]
        _CACHE["pool"] = (pts, [p.compress() for p in pts], [(-p).compress() for p in pts])
    return _CACHE["pool"]


def _inputs(K):
    """NMAX rows of K terms, the same for every test of a K (rows are prefixes): as test_gpu_msm_ct._inputs -- the edge scalars 0, 1,
    l - 1, 2^252, 2^252 - 1, all digits 8, all digits 7 at every fifth term, random ones between; the identity encoding (t = 3 mod 11), a
    repeated point (t = 7 mod 11, where the row has the term two before); rows 6, 14, .. with K >= 2 begin with P and -P under equal
    scalars.  -> (scalars [row][k] ints, points [row][k] encodings)"""
    key = ("in", K)
    if key not in _CACHE:
        _, enc, neg = _pool()
        edge = [0, 1, L - 1, 2**252, 2**252 - 1, int("8" * 63, 16), int("7" * 63, 16)]
        scalars, points = [], []
        for i in range(NMAX):
            srow, prow = [], []
            for k in range(K):
                t = i * K + k
                srow.append(edge[(t // 5) % 7] if t % 5 == 0 else int.from_bytes(_h(b"rows-s", t), "little") % L)
                if t % 11 == 3:
                    prow.append(IDENT)
                elif t % 11 == 7 and k >= 2:
                    prow.append(prow[k - 2])
                else:
                    prow.append(enc[(7 * t + 3) % 48])
            if K >= 2 and i % 8 == 6:
                j = (5 * i) % 48
                prow[0], prow[1] = enc[j], neg[j]
                srow[1] = srow[0] = edge[(i // 8) % 6 + 1]
            scalars.append(srow)
            points.append(prow)
        _CACHE[key] = (scalars, points)
    return _CACHE[key]


def _reference(engine, K, shared):
    """NMAX outputs through bpp_msm_ct_batched on host copies (shared: every row over row 0's points), once per (K, form)"""
    key = ("ref", K, shared)
    if key not in _CACHE:
        scalars, points = _inputs(K)
        s32 = [sb(s) for row in scalars for s in row]
        p32 = [p for i in range(NMAX) for p in points[0 if shared else i]]
        _CACHE[key] = engine.msm_ct_batched(s32, p32, [K * i for i in range(NMAX + 1)])
    return _CACHE[key]


def _scalar_rows(scalars):
    return _np([b"".join(sb(s) for s in row) for row in scalars])


def _point_rows(points):
    return _np([b"".join(row) for row in points])


def _record(res):
    r = res.result()
    return [r["n_done"], r["n_void"], r["first_void"], r["flags"]]


def _out(res):
    res.wait()
    return [bytes(r) for r in res.out.cpu().numpy()]


# ---------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("shared", [False, True], ids=["rows", "shared"])
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("K", KS)
def test_parity(engine, packed, K, n, shared):
    scalars, points = _inputs(K)
    want = _reference(engine, K, shared)[:n]
    pts = _dev(_point_rows(points[:1]).reshape(K, 32)) if shared else _dev(_point_rows(points[:n]))
    res = packed.rows_msm(engine, _dev(_scalar_rows(scalars[:n])), pts, K)
    assert _out(res) == want
    assert _record(res) == [n, 0, None, WRITTEN]  # valid inputs: no row is void, every row is done
    assert res.done_mask.cpu().numpy().tolist() == [1] * n


@pytest.mark.parametrize("K", [1, 2, 5, 16])
def test_the_reference_is_the_oracles(engine, K):
    """the first rows of the shared reference against the oracle's multiscalar_mul (P and -P: row 6 is the identity for K >= 2)"""
    scalars, points = _inputs(K)
    rows = (0, 1, 6)
    if ("oracle", K) not in _CACHE:
        _CACHE[("oracle", K)] = [C.multiscalar_mul(scalars[i], [C.decompress(p) for p in points[i]]).compress() for i in rows]
    want = _reference(engine, K, False)
    assert [want[i] for i in rows] == _CACHE[("oracle", K)]
    if K >= 2:
        assert want[6] == C.multiscalar_mul(scalars[6][2:], [C.decompress(p) for p in points[6][2:]]).compress()


def test_commitment_shape(bpp, engine, packed):
    """K = 2 over the exported H and G_0 == bpp_pedersen_commit (k_ct_fixed), with shared bases and with per-row points"""
    params = bpp.RangeParameters.init(8, 1, bpp.create_pedersen_gens_with_extension_degree(1), engine=engine)
    try:
        values = [0, 1, 2**64 - 1, 0x0123456789abcdef, 2**63, 7, 8, 9, 10]
        blind = [[sb(int.from_bytes(_h(b"rows-b", j), "little") % L)] for j in range(len(values))]
        blind[0], blind[1] = [sb(0)], [sb(L - 1)]
        want = params.commit_many(values, blind)
        bases = params.h_base_compressed() + params.g_bases_compressed()[0]
        scal = _dev(_np([sb(v) + b[0] for v, b in zip(values, blind)]))
        got = _out(packed.rows_msm(engine, scal, _dev(_np([bases])).reshape(2, 32), 2))
        assert got == want and got[0] == IDENT
        assert _out(packed.rows_msm(engine, scal, _dev(_np([bases] * len(values))), 2)) == want
    finally:
        params.close()


# ---------------------------------------------------------------- 2. geometry
def _strided(rows, stride, offset, fill=0xEE, tail=0):
    """uint8 [n, len] at `offset` bytes into a poisoned allocation, rows `stride` apart -> (the view, the whole buffer)"""
    n, width = rows.shape
    buf = np.full(offset + n * stride + tail, fill, dtype=np.uint8)
    for i in range(n):
        buf[offset + i * stride:offset + i * stride + width] = rows[i]
    whole = _dev(buf)
    return whole[offset:offset + n * stride].view(n, stride)[:, :width], whole


@pytest.mark.parametrize("shared", [False, True], ids=["rows", "shared"])
@pytest.mark.parametrize("K,out_stride", [(1, 32), (3, 32), (3, 45), (8, 33)])
def test_odd_addresses_and_slack(engine, packed, K, out_stride, shared):
    n = 9
    scalars, points = _inputs(K)
    want = _reference(engine, K, shared)[:n]
    sc, sc_whole = _strided(_scalar_rows(scalars[:n]), 32 * K + 5, 1)
    pt, pt_whole = _strided(_point_rows(points[:1 if shared else n]), 32 * K + 3, 3)
    out, out_whole = _strided(np.full((n, 32), 0xEE, dtype=np.uint8), out_stride, 1, tail=3)
    live_whole = _dev(np.array([7] + [1] * n, dtype=np.uint8))
    done_whole = torch.full((n + 2,), 0xEE, dtype=torch.uint8, device="cuda")
    assert sc.data_ptr() % 2 == 1 and pt.data_ptr() % 2 == 1 and out.data_ptr() % 2 == 1
    before = [t.clone() for t in (sc_whole, pt_whole)]
    res = packed.rows_msm(engine, sc, pt.reshape(K, 32) if shared and (K > 1) else pt, K, out=out, live=live_whole[1:], done_mask=done_whole[1:n + 1])
    assert _out(res) == want and _record(res) == [n, 0, None, WRITTEN]
    assert torch.equal(sc_whole, before[0]) and torch.equal(pt_whole, before[1])
    host = out_whole.cpu().numpy()
    assert host[0] == 0xEE and (host[1 + n * out_stride:] == 0xEE).all()
    assert (host[1:1 + n * out_stride].reshape(n, out_stride)[:, 32:] == 0xEE).all(), "output slack was written"
    assert done_whole.cpu().numpy().tolist() == [0xEE] + [1] * n + [0xEE]


# ---------------------------------------------------------------- 3. live mask and void rows
def _host_model(bpp, sc_rows, pt_rows, K, live, shared=False):
    """the host model of k_rows_msm (csrc/rows_msm.h: rows_msm_run_host, through libbpp_hosttest.so) -> (outputs, done_mask, record)"""
    lib = ctypes.CDLL(bpp._build.build_hosttest())
    P, Z, U = ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32
    lib.ht_rows_msm.restype = None
    lib.ht_rows_msm.argtypes = [P, Z, P, Z, Z, U, P, Z, P, P, ctypes.POINTER(U), P, Z, ctypes.POINTER(Z)]
    n = len(live)
    out, done, rec = ctypes.create_string_buffer(32 * n), ctypes.create_string_buffer(n), (U * 4)()
    lib.ht_rows_msm(sc_rows.tobytes(), 32 * K, pt_rows.tobytes(), 0 if shared else 32 * K, n, K, out, 32, bytes(live), done, rec, None, 0, None)
    r = list(rec)
    return [out.raw[32 * i:32 * i + 32] for i in range(n)], list(done.raw), [r[0], r[1], None if r[2] == 0xFFFFFFFF else r[2], r[3]]


def test_dead_rows_and_sources_that_end_behind_the_last_live_row(engine, packed):
    K, n, last_live = 3, 12, 8
    scalars, points = _inputs(K)
    want = _reference(engine, K, False)
    live = [1, 0, 1, 1, 0, 1, 1, 0, 1, 0, 0, 0]
    sc_rows, pt_rows = _scalar_rows(scalars[:last_live + 1]), _point_rows(points[:last_live + 1])
    for i in range(last_live + 1):
        if not live[i]:  # dead rows: scalars >= l and undecodable points, which would void a live row
            sc_rows[i, :], pt_rows[i, :] = 0xFF, 0xFF
    # ONE allocation: what the call writes in front, then the points and, ending with the allocation, the scalars -- both sources END
    # behind row 8; rows 9 .. 11 exist in the mask and in the outputs alone (the ranges the call is told of reach past the sources'
    # ends, over memory it only reads)
    w = 32 * K
    o_out, o_done, o_rec, o_live, o_pt = 0, 12 * 32, 400, 416, 432
    o_sc = o_pt + (last_live + 1) * w
    buf = np.full(o_sc + (last_live + 1) * w, 0xEE, dtype=np.uint8)
    buf[o_live:o_live + n] = live
    buf[o_pt:o_sc] = pt_rows.reshape(-1)
    buf[o_sc:] = sc_rows.reshape(-1)
    whole = _dev(buf)
    base = whole.data_ptr()
    res = packed.rows_msm(engine, (base + o_sc, (n, w), w), (base + o_pt, (n, w), w), K, out=whole[o_out:o_out + n * 32].view(n, 32),
                          live=whole[o_live:o_live + n], done_mask=whole[o_done:o_done + n], record=whole[o_rec:o_rec + 16].view(torch.int32))
    res.wait()
    assert torch.equal(whole[o_live:], _dev(buf[o_live:]))  # the inputs are as they were
    assert _out(res) == [want[i] if live[i] else IDENT for i in range(n)]
    assert _record(res) == [sum(live), 0, None, WRITTEN]
    assert res.done_mask.cpu().numpy().tolist() == live


def test_void_rows(bpp, engine, packed):
    K, n = 3, 10
    scalars, points = _inputs(K)
    scalars, points = [list(r) for r in scalars[:n]], [list(r) for r in points[:n]]
    want = _reference(engine, K, False)
    live = [1] * n
    live[0] = 0
    scalars[0][0], points[0][0] = 2**256 - 1, BAD_POINT       # dead: counts for nothing
    scalars[3][K - 1] = L                                      # a scalar >= l in the LAST term
    points[5][1] = BAD_POINT                                   # a point that does not decode
    scalars[7][0], points[7][2] = 2**256 - 1, b"\xff" * 32     # both
    sc_np, pt_np = _np([b"".join(s.to_bytes(32, "little") for s in row) for row in scalars]), _point_rows(points)
    sc, pt = _dev(sc_np), _dev(pt_np)
    res = packed.rows_msm(engine, sc, pt, K, live=_dev(np.array(live, dtype=np.uint8)))
    done = [0, 1, 1, 0, 1, 0, 1, 0, 1, 1]
    assert (_out(res), res.done_mask.cpu().numpy().tolist(), _record(res)) == _host_model(bpp, sc_np, pt_np, K, live)
    assert _out(res) == [want[i] if done[i] else IDENT for i in range(n)]
    assert res.done_mask.cpu().numpy().tolist() == done
    assert _record(res) == [6, 3, 3, WRITTEN | SCALAR | POINT]  # the lowest index wins; both flags
    # each cause alone
    for rows_live, rec in (((3, 4), [1, 1, 3, WRITTEN | SCALAR]), ((5, 6), [1, 1, 5, WRITTEN | POINT]), ((7,), [0, 1, 7, WRITTEN | SCALAR | POINT])):
        lv = np.zeros(n, dtype=np.uint8)
        lv[list(rows_live)] = 1
        assert _record(packed.rows_msm(engine, sc, pt, K, live=_dev(lv))) == rec
    # a shared base that does not decode voids every live row (their scalars are canonical), and only those
    lv = np.array([1, 1, 1, 0, 1, 1, 1, 0, 1, 1], dtype=np.uint8)
    lv[0] = 0
    res = packed.rows_msm(engine, sc, _dev(_np([b"".join(points[5])])).reshape(K, 32), K, live=_dev(lv))
    assert _out(res) == [IDENT] * n and res.done_mask.cpu().numpy().tolist() == [0] * n
    assert _record(res) == [0, 7, 1, WRITTEN | POINT]
    assert ([IDENT] * n, [0] * n, _record(res)) == _host_model(bpp, sc_np, _np([b"".join(points[5])]), K, lv.tolist(), shared=True)


# ---------------------------------------------------------------- 4. the scalar operation
def _scalars_np(vals):
    return _np([int(v).to_bytes(32, "little") for v in vals])


def _ints(res):
    return [int.from_bytes(b, "little") for b in _out(res)]


def test_scalar_operation(engine, packed):
    edge = [0, 1, L - 1, 2**252, 2**252 - 1] + [int.from_bytes(_h(b"rows-m", i), "little") % L for i in range(6)]
    a = [x for x in edge for _ in edge]
    b = [y for _ in edge for y in edge]
    c = [edge[(3 * i + 1) % len(edge)] for i in range(len(a))]
    n = len(a)  # 121: two workgroups of 64 lanes, the second partly idle
    A, _ = _strided(_scalars_np(a), 37, 1)
    B, _ = _strided(_scalars_np(b), 32, 3)
    Cc, _ = _strided(_scalars_np(c), 33, 1)
    out, out_whole = _strided(np.full((n, 32), 0xEE, dtype=np.uint8), 35, 1, tail=2)
    res = packed.rows_scalar_muladd(engine, A, B, Cc, out=out)
    assert _ints(res) == [(x * y + z) % L for x, y, z in zip(a, b, c)]
    assert _record(res) == [n, 0, None, WRITTEN] and res.done_mask.cpu().numpy().tolist() == [1] * n
    host = out_whole.cpu().numpy()
    assert host[0] == 0xEE and (host[1 + n * 35:] == 0xEE).all() and (host[1:1 + n * 35].reshape(n, 35)[:, 32:] == 0xEE).all()
    # c = NULL
    assert _ints(packed.rows_scalar_muladd(engine, A, B)) == [(x * y) % L for x, y in zip(a, b)]
    # one scalar for every row (stride 0), in each position
    one = lambda v: _dev(_scalars_np([v]))  # noqa: E731
    assert _ints(packed.rows_scalar_muladd(engine, one(a[17]), B, Cc)) == [(a[17] * y + z) % L for y, z in zip(b, c)]
    assert _ints(packed.rows_scalar_muladd(engine, A, one(b[5]), Cc)) == [(x * b[5] + z) % L for x, z in zip(a, c)]
    assert _ints(packed.rows_scalar_muladd(engine, A, B, one(c[2]))) == [(x * y + c[2]) % L for x, y in zip(a, b)]
    assert _ints(packed.rows_scalar_muladd(engine, A, B, one(c[2]).reshape(32))) == [(x * y + c[2]) % L for x, y in zip(a, b)]


def test_scalar_operation_void_and_dead_rows(engine, packed):
    a, b, c = [3, L, 4, 5, 6, 7, 2], [8, 9, 2**256 - 1, 10, 11, L, 2], [12, 13, 14, L + 1, 15, 2**256 - 1, 2]
    live = [1, 1, 1, 1, 1, 0, 1]
    res = packed.rows_scalar_muladd(engine, _dev(_scalars_np(a)), _dev(_scalars_np(b)), _dev(_scalars_np(c)),
                                    live=_dev(np.array(live, dtype=np.uint8)))
    assert _ints(res) == [(3 * 8 + 12) % L, 0, 0, 0, (6 * 11 + 15) % L, 0, 6]
    assert res.done_mask.cpu().numpy().tolist() == [1, 0, 0, 0, 1, 0, 1]
    assert _record(res) == [3, 3, 1, WRITTEN | SCALAR]
    # a broadcast operand that is not canonical voids every live row
    res = packed.rows_scalar_muladd(engine, _dev(_scalars_np([3, 4, 5])), _dev(_scalars_np([L])), live=_dev(np.array([1, 0, 1], dtype=np.uint8)))
    assert _ints(res) == [0, 0, 0] and _record(res) == [0, 2, 0, WRITTEN | SCALAR]


# ---------------------------------------------------------------- 5. refusals
def _raw_msm(bpp, engine, n, K, s, ss, p, ps, o, os_, live=None, done=None, rec=None):
    lib_mod = importlib.import_module("bulletproofs-plus_amd._lib")
    api = importlib.import_module("bulletproofs-plus_amd.api")
    desc = lib_mod.RowsMsm(n, K, s, ss, p, ps)
    api._check(engine.lib.bpp_rows_msm_enqueue(engine.ctx, ctypes.byref(desc), o, os_, live, done, rec, None), engine.ctx)


def _raw_scalar(engine, n, a, b, c, o, os_, live=None, done=None, rec=None):
    lib_mod = importlib.import_module("bulletproofs-plus_amd._lib")
    api = importlib.import_module("bulletproofs-plus_amd.api")
    ops = [None if x is None else lib_mod.ScalarRows(*x) for x in (a, b, c)]
    ref = [None if x is None else ctypes.byref(x) for x in ops]
    api._check(engine.lib.bpp_rows_scalar_enqueue(engine.ctx, n, ref[0], ref[1], ref[2], o, os_, live, done, rec, None), engine.ctx)


def test_refusals(bpp, engine, packed):
    buf = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr()
    s, p, o, lv, dm, rc = base, base + 1024, base + 2048, base + 3000, base + 3100, base + 3200
    host = np.zeros(4096, dtype=np.uint8)
    _raw_msm(bpp, engine, 4, 2, s, 64, p, 64, o, 32, lv, dm, rc)  # the arguments the refusals vary are fine
    torch.cuda.synchronize()
    calls = packed.rows_stats(engine)["calls"]
    msm_cases = [
        ((0, 2, s, 64, p, 64, o, 32, lv, dm, rc), "n is 0"),
        ((2**31, 2, s, 64, p, 64, o, 32, lv, dm, rc), "n is above 2^31 - 1"),
        ((4, 0, s, 64, p, 64, o, 32, lv, dm, rc), "K must be 1 .. 16"),
        ((4, 17, s, 544, p, 544, o, 32, lv, dm, rc), "K must be 1 .. 16"),
        ((4, 2, s, 63, p, 64, o, 32, lv, dm, rc), "scalar_stride is below 32 K"),
        ((4, 2, s, 64, p, 63, o, 32, lv, dm, rc), "point_stride is below 32 K"),
        ((4, 2, s, 64, p, 64, o, 31, lv, dm, rc), "out_stride is below 32"),
        ((4, 2, None, 64, p, 64, o, 32, lv, dm, rc), "scalars_dev is null"),
        ((4, 2, s, 64, None, 64, o, 32, lv, dm, rc), "points_dev is null"),
        ((4, 2, s, 64, p, 64, None, 32, lv, dm, rc), "out_dev is null"),
        ((4, 2, host.ctypes.data, 64, p, 64, o, 32, lv, dm, rc), "scalars_dev is not device memory of this context's device"),
        ((4, 2, s, 64, host.ctypes.data, 64, o, 32, lv, dm, rc), "points_dev is not device memory of this context's device"),
        ((4, 2, s, 64, p, 64, host.ctypes.data, 32, lv, dm, rc), "out_dev is not device memory of this context's device"),
        ((4, 2, s, 64, p, 64, o, 32, host.ctypes.data, dm, rc), "live_dev is not device memory of this context's device"),
        ((4, 2, s, 64, p, 64, o, 32, lv, host.ctypes.data, rc), "done_mask_dev is not device memory of this context's device"),
        ((4, 2, s, 64, p, 64, o, 32, lv, dm, host.ctypes.data), "record_dev is not device memory of this context's device"),
        ((4, 2, s, 64, p, 64, s + 255, 32, lv, dm, rc), "scalars_dev and out_dev overlap"),
        ((4, 2, s, 64, p, 64, p + 63, 32, lv, dm, rc), "points_dev and out_dev overlap"),
        ((4, 2, s, 64, p, 64, o, 32, lv, o + 127, rc), "out_dev and done_mask_dev overlap"),
        ((4, 2, s, 64, p, 64, o, 32, lv, lv + 3, rc), "live_dev and done_mask_dev overlap"),
        ((4, 2, s, 64, p, 64, o, 32, lv, dm, o + 100), "out_dev and record_dev overlap"),
        ((4, 2, s, 64, p, 64, o, 32, lv, dm, dm + 3), "done_mask_dev and record_dev overlap"),
    ]
    for args, msg in msm_cases:
        with pytest.raises(bpp.ProofError) as e:
            _raw_msm(bpp, engine, *args)
        assert e.value.kind == bpp.ProofErrorKind.InvalidArgument and msg in str(e.value), (msg, str(e.value))
    A, B, Cc = (s, 32), (p, 32), (base + 4096, 32)
    scalar_cases = [
        ((0, A, B, Cc, o, 32), "n is 0"),
        ((4, (None, 32), B, Cc, o, 32), "a.dev is null"),
        ((4, A, (p, 31), Cc, o, 32), "b.stride is below 32"),
        ((4, A, B, Cc, None, 32), "out_dev is null"),
        ((4, A, B, Cc, o, 16), "out_stride is below 32"),
        ((4, (host.ctypes.data, 32), B, Cc, o, 32), "a.dev is not device memory of this context's device"),
        ((4, A, B, (host.ctypes.data, 0), o, 32), "c.dev is not device memory of this context's device"),
        ((4, A, B, Cc, s, 32), "a.dev and out_dev overlap"),          # out may alias none of the inputs
        ((4, A, B, Cc, p + 127, 32), "b.dev and out_dev overlap"),
        ((4, A, B, (o + 31, 0), o, 32), "c.dev and out_dev overlap"),
    ]
    for args, msg in scalar_cases:
        with pytest.raises(bpp.ProofError) as e:
            _raw_scalar(engine, *args, lv, dm, rc)
        assert e.value.kind == bpp.ProofErrorKind.InvalidArgument and msg in str(e.value), (msg, str(e.value))
    assert packed.rows_stats(engine)["calls"] == calls  # a refused call counts for nothing
    _raw_scalar(engine, 4, A, B, None, o, 32, lv, dm, rc)
    assert packed.rows_stats(engine)["calls"] == calls + 1
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 6. steady state
@pytest.mark.parametrize("shared", [False, True], ids=["rows", "shared"])
def test_steady_state(engine, packed, shared):
    K, n = 2, 33
    scalars, points = _inputs(K)
    sc = _dev(_scalar_rows(scalars[:n]))
    pt = _dev(_point_rows(points[:1]).reshape(K, 32)) if shared else _dev(_point_rows(points[:n]))
    out = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    x = _dev(_scalars_np([5] * n))
    first = packed.rows_msm(engine, sc, pt, K, out=out)
    before = packed.rows_stats(engine)
    last = None
    for _ in range(10):
        last = packed.rows_msm(engine, sc, pt, K, out=out)
        packed.rows_scalar_muladd(engine, x, x, None)
    after = packed.rows_stats(engine)
    assert after["calls"] == before["calls"] + 20
    assert after["first_calls"] == before["first_calls"] and after["host_waits"] == before["host_waits"] == 0
    assert first.ticket < last.ticket
    assert _out(last) == _reference(engine, K, shared)[:n]
    assert first.done()


# ---------------------------------------------------------------- 7. the step, end to end
def test_commit_challenge_response_on_the_stream(engine, packed):
    """a Schnorr proof of knowledge of x (X = x G) bound to a transcript, n = 9 rows on one stream with ONE wait at the end: row 4 is dead,
    row 6 has the identity as its public key X and is void from the APPEND_POINT on."""
    n, dead, ident = 9, 4, 6
    G = C.BASEPOINT.compress()
    x = [int.from_bytes(_h(b"rows-x", i), "little") % L for i in range(n)]
    x[ident] = 0
    X = [(C.BASEPOINT * v).compress() for v in x]
    assert X[ident] == IDENT
    txid = [_h(b"rows-txid", i, 24) for i in range(n)]
    live_l = [0 if i == dead else 1 for i in range(n)]
    live = _dev(np.array(live_l, dtype=np.uint8))
    states = torch.full((n, 203), 0xEE, dtype=torch.uint8, device="cuda")
    d_x, d_X, d_txid = _dev(_scalars_np(x)), _dev(_np(X)), _dev(_np(txid))
    proto = b"rows step"
    waits = packed.transcripts_stats(engine)["host_waits"]
    # 1 + 2: the transcript, and r from its RNG (keyed with the witness x)
    t1 = packed.transcript_ops(engine, states, [packed.TNew(proto), packed.TAppend(b"txid", d_txid), packed.TRngBegin(),
                                                packed.TRngRekey(b"x", d_x), packed.TRngFinalize(None), packed.TRngScalars(1)], live=live)
    r = t1.outputs[0]
    # 3: R = r G
    m = packed.rows_msm(engine, r, _dev(_np([G])), 1, live=live)
    # 4: X, R into the transcript, the challenge out of it
    t2 = packed.transcript_ops(engine, states, [packed.TAppendPoint(b"X", d_X), packed.TAppendPoint(b"R", m.out), packed.TChallengeScalar(b"c")],
                               live=live)
    c = t2.outputs[0]
    # 5: s = c x + r on the rows the transcript call advanced (its done mask is this call's live mask: a void row answers nothing)
    s = packed.rows_scalar_muladd(engine, c, d_x, r, live=t2.done_mask)
    s.wait()  # the one wait
    assert t1.done() and m.done() and t2.done()
    assert packed.transcripts_stats(engine)["host_waits"] == waits

    r_h, R_h, c_h, s_h = ([bytes(v) for v in t.cpu().numpy()] for t in (r, m.out, c, s.out))
    st_h = [bytes(v) for v in states.cpu().numpy()]
    # the host helpers on host copies: the same program, R taken from the oracle
    fresh = []
    for _ in range(n):
        b = (ctypes.c_uint8 * 203)()
        assert engine.lib.bpp_transcript_new((ctypes.c_uint8 * len(proto)).from_buffer_copy(proto), len(proto), b) == 0
        fresh.append(bytes(b))
    prog1 = [("append", b"txid", txid), ("begin",), ("rekey", b"x", [sb(v) for v in x]), ("finalize", None), ("scalars", 1)]
    h_states1, h_outs1, h_void1 = TC.helper_rows(engine.lib, fresh, prog1)
    assert not any(h_void1)
    want_r = h_outs1[0]
    want_R = [(C.BASEPOINT * int.from_bytes(v, "little")).compress() for v in want_r]
    prog2 = [("point", b"X", X), ("point", b"R", want_R), ("cscalar", b"c")]
    h_states2, h_outs2, h_void2 = TC.helper_rows(engine.lib, h_states1, prog2)
    assert h_void2 == [i == ident for i in range(n)]
    for i in range(n):
        if i == dead:  # never touched; every output zero
            assert st_h[i] == b"\xee" * 203 and r_h[i] == R_h[i] == c_h[i] == s_h[i] == IDENT
            continue
        assert r_h[i] == want_r[i] and R_h[i] == want_R[i]
        if i == ident:  # void from the APPEND_POINT on: the row, the challenge and the response are zero
            assert st_h[i] == bytes(203) and c_h[i] == IDENT and s_h[i] == IDENT
            continue
        assert st_h[i] == h_states2[i] and c_h[i] == h_outs2[0][i]
        ri, ci, si = (int.from_bytes(v[i], "little") for v in (r_h, c_h, s_h))
        assert si == (ci * x[i] + ri) % L
        assert (C.BASEPOINT * si).compress() == (C.decompress(R_h[i]) + C.decompress(X[i]) * ci).compress()  # s G == R + c X
    assert _record(m) == [n - 1, 0, None, WRITTEN]
    assert t2.result() == {"n_done": n - 2, "n_void": 1, "first_void": ident, "flags": WRITTEN | 2}
    assert _record(s) == [n - 2, 0, None, WRITTEN]
    assert s.done_mask.cpu().numpy().tolist() == [int(i not in (dead, ident)) for i in range(n)]
