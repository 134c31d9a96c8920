"""GPU tests of the transcript protocol and the transcript RNG on device rows (bpp_transcripts_enqueue / packed.transcript_ops with
TAppendPoint, TChallengeScalar, TRngBegin, TRngRekey, TRngFinalize, TRngFill, TRngFill32, TRngScalars).

Every expected byte comes from oracle.pyref: merlin's build_rng / rekey_with_witness_bytes / finalize / fill_bytes with NullRng and
ByteStreamRng, protocol._challenge_scalar and _validate_and_append_point, curve.scalar_from_wide (tests/transcript_rng_cases.py runs a
program on them row by row).  The shapes are the smallest at which the kernel can go wrong: every starting position of the block,
witness and fill lengths on either side of the rate and of the 256-byte LDS chunk, scalar counts on either side of the four draws
reduced at once, rows at odd addresses with slack, one row and either side of a wavefront's worth."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from oracle.pyref import curve as C
from oracle.pyref import merlin as M
from oracle.pyref import protocol as O
from tests import transcript_rng_cases as TC

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = 2
WRITTEN, IDENTITY, ZERO_SCALAR = 1, 2, 4
READS = ("append", "point", "rekey")


@pytest.fixture(scope="module")
def packed():
    return importlib.import_module("bulletproofs-plus_amd.packed")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _states(makers):
    return np.stack([np.frombuffer(mk().strobe.to_bytes(), dtype=np.uint8) for mk in makers]).copy()


def _rows(msgs, width=None, fill=0xEE):
    width = max(len(b) for b in msgs) if width is None else width
    arr = np.full((len(msgs), width), fill, dtype=np.uint8)
    for i, b in enumerate(msgs):
        arr[i, :len(b)] = np.frombuffer(b, dtype=np.uint8)
    return arr


def _ops(packed, prog, n, lens=False, cap=None, new=None):
    """the device form of a program of tests/transcript_rng_cases.py"""
    ops = [packed.TNew(new)] if new is not None else []
    for op in prog:
        kind = op[0]
        if kind == "point":
            ops.append(packed.TAppendPoint(op[1], _dev(_rows(op[2]))))
        elif kind in READS:
            arr = _rows(op[2], cap if lens else None)
            ten = _dev(arr) if arr.shape[1] else None
            ln = _dev(np.array([len(b) for b in op[2]], dtype=np.int32)) if lens else None
            ops.append((packed.TAppend if kind == "append" else packed.TRngRekey)(op[1], ten, ln))
        elif kind == "begin":
            ops.append(packed.TRngBegin())
        elif kind == "finalize":
            ops.append(packed.TRngFinalize(None if op[1] is None else _dev(_rows(op[1]))))
        else:
            w = TC.out_width(op)
            out = torch.full((n, w), 0xFF, dtype=torch.uint8, device="cuda") if w else None
            if kind == "challenge":
                ops.append(packed.TChallenge(op[1], w, out))
            elif kind == "cscalar":
                ops.append(packed.TChallengeScalar(op[1], out))
            elif kind == "fill":
                ops.append(packed.TRngFill(w, out))
            elif kind == "fill32":
                ops.append(packed.TRngFill32(w, out))
            else:
                ops.append(packed.TRngScalars(op[1], out))
    return ops


def _hold(res, want, what="", start=None, dead=()):
    """the device's rows and outputs against (states, outs, void) of the oracle; void rows are zero everywhere, dead rows keep their
    state (start) and have zero outputs"""
    res.wait()
    w_states, w_outs, w_void = want
    got = res.states.cpu().numpy()
    for i in range(len(w_states)):
        if i in dead:
            assert np.array_equal(got[i], start[i]), "%s: dead row %d was written" % (what, i)
        elif w_void[i]:
            assert not got[i].any(), "%s: void row %d is not zero" % (what, i)
        else:
            assert bytes(got[i]) == w_states[i], "%s: state row %d differs from the oracle's" % (what, i)
    assert len(res.outputs) == len(w_outs)
    for c, w in enumerate(w_outs):
        if not len(w[0]):
            continue
        out = res.outputs[c].cpu().numpy()
        for i in range(len(w)):
            if i in dead or w_void[i]:
                assert not out[i].any(), "%s: output %d of row %d is not zero" % (what, c, i)
            else:
                assert bytes(out[i]) == w[i], "%s: output %d differs from the oracle's in row %d" % (what, c, i)
    live_done = [int(not (i in dead or w_void[i])) for i in range(len(w_states))]
    assert list(res.done_mask.cpu().numpy()) == live_done, what


# ---------------------------------------------------------------- 1. every starting position
def test_every_starting_position(engine, packed):
    makers = TC.sweep_makers()
    n = len(makers)
    assert n == 169
    prog = TC.sweep_program(n)
    want = TC.oracle_rows(makers, prog)
    res = packed.transcript_ops(engine, _dev(_states(makers)), _ops(packed, prog, n))
    _hold(res, want, "169 rows")
    # the RNG operations left the rows untouched: the oracle's transcripts after challenge_scalar alone
    alone = TC.oracle_rows(makers, [("cscalar", b"e")])
    assert [bytes(r) for r in res.states.cpu().numpy()] == alone[0]
    assert res.done_mask.cpu().numpy().all()
    assert res.result() == {"n_done": n, "n_void": 0, "first_void": None, "flags": WRITTEN}


# ---------------------------------------------------------------- 2. either side of the rate and of the LDS chunk
def test_lengths_either_side_of_the_rate_and_the_chunk(engine, packed):
    makers = TC.edge_makers()
    n = len(makers)
    start = _dev(_states(makers))
    for name, prog, lens in TC.length_programs(n):
        res = packed.transcript_ops(engine, start.clone(), _ops(packed, prog, n, lens=lens, cap=400))
        _hold(res, TC.oracle_rows(makers, prog), name)
        assert res.result()["n_done"] == n


# ---------------------------------------------------------------- 3. the builder's semantics
def test_the_builder_call_for_call(engine, packed):
    makers = TC.edge_makers()
    n = len(makers)
    start = _dev(_states(makers))
    got = {}
    for name, prog, new in TC.builder_programs(n):
        states = torch.full((n, 203), 0xFF, dtype=torch.uint8, device="cuda") if new is not None else start.clone()
        res = packed.transcript_ops(engine, states, _ops(packed, prog, n, new=new))
        _hold(res, TC.oracle_rows(makers, prog, new=new), name)
        got[name] = (res.states.cpu().numpy(), [o.cpu().numpy() for o in res.outputs])
    between, plain = got["transcript ops between finalize and fill"], got["the same without them"]
    assert np.array_equal(between[1][-1], plain[1][-1]) and not np.array_equal(between[0], plain[0])
    assert not np.array_equal(got["fill32 of 64"][1][0], got["fill of 64"][1][0])


# ---------------------------------------------------------------- 4. validate_and_append_point
def test_append_point_voids_the_identity(engine, packed):
    makers = TC.edge_makers()[:8]
    n = len(makers)
    points = TC.messages(400, n, [32] * n)
    prog = [("point", b"P", points), ("begin",), ("finalize", None), ("fill", 16), ("cscalar", b"e")]
    clean = packed.transcript_ops(engine, _dev(_states(makers)), _ops(packed, prog, n))
    _hold(clean, TC.oracle_rows(makers, prog), "no identity")
    assert clean.result() == {"n_done": n, "n_void": 0, "first_void": None, "flags": WRITTEN}
    as_append = TC.oracle_rows(makers, [("append", b"P", points)] + prog[1:])
    points[5] = points[2] = bytes(32)
    want = TC.oracle_rows(makers, prog)
    assert want[2] == [i in (2, 5) for i in range(n)]
    res = packed.transcript_ops(engine, _dev(_states(makers)), _ops(packed, prog, n))
    _hold(res, want, "two identities")
    assert res.result() == {"n_done": n - 2, "n_void": 2, "first_void": 2, "flags": WRITTEN | IDENTITY}
    for i in (0, 1, 3, 4, 6, 7):
        assert want[0][i] == as_append[0][i] and want[1][1][i] == as_append[1][1][i], "a point that is no identity is a plain append"


# ---------------------------------------------------------------- 5. dead and void rows
def test_dead_and_void_rows(engine, packed):
    makers = [TC.at(k, (0, 1, 2, 3, 164, 5, 165, 83, 7)[k]) for k in range(9)]
    rows = _states(makers)
    rows[2] = 0  # the zero row of a rejected item: cur_flags == 0
    rows[3] = 0xFF
    rows[3, 200], rows[3, 202] = 166, 2
    live = np.array([0, 1, 1, 1, 0, 1, 1, 1, 0], dtype=np.uint8)
    n, cap = 9, 40
    wit = TC.messages(500, n, [24] * n)
    ent = TC.messages(501, n, [32] * n)
    prog = [("begin",), ("rekey", b"w", wit), ("finalize", ent), ("fill", 300), ("fill32", 64), ("scalars", 5), ("cscalar", b"e")]
    want = TC.oracle_rows(makers, prog)
    ops = _ops(packed, prog, n)
    lengths = [24] * n
    lengths[6] = cap + 1  # beyond the cap on a valid row's REKEY
    # what a dead or void row's inputs hold must not matter: 0xFF there
    unread = [0, 2, 3, 4, 6, 8]
    wdata, edata = _rows(wit, cap, 0xFF), _rows(ent)
    wdata[unread], edata[unread] = 0xFF, 0xFF
    ops[1] = packed.TRngRekey(b"w", _dev(wdata), _dev(np.array(lengths, dtype=np.int32)))
    ops[2] = packed.TRngFinalize(_dev(edata))
    void = [2, 3, 6]
    want = (want[0], want[1], [i in void for i in range(n)])
    res = packed.transcript_ops(engine, _dev(rows), ops, live=_dev(live))
    _hold(res, want, "dead and void", start=rows, dead=(0, 4, 8))
    assert res.result() == {"n_done": 3, "n_void": 3, "first_void": 2, "flags": WRITTEN}


def test_all_dead_and_all_void(engine, packed):
    n = 5
    makers = [TC.at(k, k) for k in range(n)]
    rows = _states(makers)
    prog = [("begin",), ("rekey", b"w", TC.messages(510, n, [32] * n)), ("finalize", None), ("fill32", 32), ("scalars", 2)]
    res = packed.transcript_ops(engine, _dev(rows), _ops(packed, prog, n), live=torch.zeros(n, dtype=torch.uint8, device="cuda"),
                                done_mask=torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda"))
    assert res.result() == {"n_done": 0, "n_void": 0, "first_void": None, "flags": WRITTEN}
    assert np.array_equal(res.states.cpu().numpy(), rows) and not res.done_mask.cpu().numpy().any()
    assert all(not o.cpu().numpy().any() for o in res.outputs) and len(res.outputs) == 2
    res = packed.transcript_ops(engine, torch.zeros((n, 203), dtype=torch.uint8, device="cuda"), _ops(packed, prog, n),
                                done_mask=torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda"))
    assert res.result() == {"n_done": 0, "n_void": n, "first_void": 0, "flags": WRITTEN}
    assert not res.states.cpu().numpy().any() and not res.done_mask.cpu().numpy().any()
    assert all(not o.cpu().numpy().any() for o in res.outputs)


# ---------------------------------------------------------------- 6. geometry
@pytest.mark.parametrize("n", [1, 63, 64, 65])
@pytest.mark.parametrize("offset", [1, 3])
def test_rows_at_odd_addresses_with_slack(engine, packed, n, offset):
    makers = [TC.at(k, (37 * k) % 166) for k in range(n)]
    rows = _states(makers)
    wit, ent = TC.messages(600 + n, n, [32] * n), TC.messages(700 + n, n, [32] * n)
    prog = [("begin",), ("rekey", b"w", wit), ("finalize", ent), ("fill32", 64), ("scalars", 1), ("cscalar", b"e")]
    want = TC.oracle_rows(makers, prog)
    sbuf = torch.full((offset + n * 203 + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    sbuf[offset:offset + n * 203] = _dev(rows).reshape(-1)
    states = sbuf[offset:offset + n * 203].view(n, 203)
    assert states.data_ptr() % 4 == offset

    def slab(width, data=None):
        """rows of `width` bytes, one byte of slack each, at an odd address: (buffer, the tuple form that names the stride)"""
        buf = torch.full((1 + n * (width + 1) + 16,), 0xEE, dtype=torch.uint8, device="cuda")
        if data is not None:
            padded = np.full((n, width + 1), 0xEE, dtype=np.uint8)
            padded[:, :width] = _rows(data)
            buf[1:1 + n * (width + 1)] = _dev(padded).reshape(-1)
        assert (buf.data_ptr() + 1) % 2 == 1
        return buf, (buf.data_ptr() + 1, (n, width), width + 1)

    wbuf, wrows = slab(32, wit)
    ebuf, erows = slab(32, ent)
    outs = [slab(64), slab(32), slab(32)]
    before = [wbuf.cpu().numpy().copy(), ebuf.cpu().numpy().copy()]
    torch.cuda.synchronize()
    res = packed.transcript_ops(engine, states, [packed.TRngBegin(), packed.TRngRekey(b"w", wrows), packed.TRngFinalize(erows),
                                                 packed.TRngFill32(64, outs[0][1]), packed.TRngScalars(1, outs[1][1]),
                                                 packed.TChallengeScalar(b"e", outs[2][1])])
    res.wait()
    s = sbuf.cpu().numpy()
    assert [bytes(r) for r in s[offset:offset + n * 203].reshape(n, 203)] == want[0]
    assert (s[:offset] == 0xEE).all() and (s[offset + n * 203:] == 0xEE).all(), "a byte outside the rows was written"
    for c, ((buf, _), width) in enumerate(zip(outs, (64, 32, 32))):
        o = buf.cpu().numpy()
        got = o[1:1 + n * (width + 1)].reshape(n, width + 1)
        assert [bytes(r[:width]) for r in got] == want[1][c], "output %d" % c
        assert (got[:, width] == 0xEE).all() and o[0] == 0xEE and (o[1 + n * (width + 1):] == 0xEE).all(), "slack of output %d was written" % c
    assert np.array_equal(wbuf.cpu().numpy(), before[0]) and np.array_equal(ebuf.cpu().numpy(), before[1])
    assert res.result() == {"n_done": n, "n_void": 0, "first_void": None, "flags": WRITTEN}


# ---------------------------------------------------------------- 7. refusals
def test_refusals_before_any_launch(engine, packed):
    lib, T, P = engine.lib, packed._lib.TranscriptOp, packed
    n = 4
    states = torch.zeros((n, 203), dtype=torch.uint8, device="cuda")
    wit = torch.zeros((n, 40), dtype=torch.uint8, device="cuda")
    ent = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    out = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
    out2 = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
    pts = torch.ones((n, 32), dtype=torch.uint8, device="cuda")
    lens = torch.zeros((n,), dtype=torch.int32, device="cuda")
    live = torch.ones((n,), dtype=torch.uint8, device="cuda")
    done = torch.zeros((n,), dtype=torch.uint8, device="cuda")
    rec = torch.zeros((4,), dtype=torch.int32, device="cuda")
    label = (ctypes.c_uint8 * 400)()
    lab = ctypes.addressof(label)
    host = np.zeros(4096, dtype=np.uint8)  # host memory: never dereferenced

    def base():
        ops = (T * 9)()
        ops[0] = T(P.TOP_RNG_BEGIN, None, 0, None, 0, 0, None)
        ops[1] = T(P.TOP_RNG_REKEY, lab, 3, wit.data_ptr(), 40, 40, lens.data_ptr())
        ops[2] = T(P.TOP_RNG_FINALIZE, None, 0, ent.data_ptr(), 32, 32, None)
        ops[3] = T(P.TOP_RNG_FILL32, None, 0, out.data_ptr(), 64, 64, None)
        ops[4] = T(P.TOP_RNG_SCALARS, None, 0, out2.data_ptr(), 64, 64, None)
        return ops

    def call(ops, n_ops=5):
        rc = lib.bpp_transcripts_enqueue(engine.ctx, ctypes.c_void_p(states.data_ptr()), n, ops, n_ops, ctypes.c_void_p(live.data_ptr()),
                                         ctypes.c_void_p(done.data_ptr()), ctypes.c_void_p(rec.data_ptr()), None)
        return rc, lib.bpp_ctx_last_error(engine.ctx).decode()

    def refused(needle, ops, **kw):
        rc, msg = call(ops, **kw)
        assert rc == INVALID_ARGUMENT and needle in msg, (needle, rc, msg)

    def accepted(ops, **kw):
        rc, msg = call(ops, **kw)
        assert rc == 0, msg

    point = lambda kind, data=pts: T(kind, lab, 1, data.data_ptr(), 32, 32, None)  # noqa: E731
    torch.cuda.synchronize()
    accepted(base())
    before = packed.transcripts_stats(engine)
    for k in (0, 4, 7, 15, 18, 31, 38):
        ops = base(); ops[4].kind = k; refused("ops[4].kind", ops)
    # len other than 32
    for kind in (P.TOP_APPEND_POINT, P.TOP_CHALLENGE_SCALAR):
        ops = base(); ops[4] = point(kind, out2); ops[4].len = 31; refused("ops[4].len", ops)
        ops = base(); ops[4] = point(kind, out2); ops[4].len, ops[4].stride = 64, 64; refused("ops[4].len", ops)
    ops = base(); ops[2].len = 16; refused("ops[2].len", ops)
    ops = base(); ops[2].len = 0; refused("ops[2].len", ops)
    # len not a multiple of 32
    ops = base(); ops[3].len = 48; refused("ops[3].len", ops)
    ops = base(); ops[4].len = 33; refused("ops[4].len", ops)
    # lens_dev on anything but APPEND / RNG_REKEY
    for j in (2, 3, 4):
        ops = base(); ops[j].lens_dev = lens.data_ptr(); refused("ops[%d].lens_dev" % j, ops)
    ops = base(); ops[4] = point(P.TOP_APPEND_POINT); ops[4].lens_dev = lens.data_ptr(); refused("ops[4].lens_dev", ops)
    # RNG_BEGIN with a label or data
    ops = base(); ops[0].label, ops[0].label_len = lab, 1; refused("ops[0].label", ops)
    ops = base(); ops[0].data_dev = pts.data_ptr(); refused("ops[0].data_dev", ops)
    # the order of the RNG operations
    ops = base(); ops[0] = point(P.TOP_APPEND_POINT); refused("ops[1].kind", ops)
    ops = base(); ops[1], ops[2] = ops[2], T(P.TOP_RNG_REKEY, lab, 3, wit.data_ptr(), 40, 40, None); refused("ops[2].kind", ops)
    ops = base(); ops[3] = T(P.TOP_RNG_FINALIZE, None, 0, None, 0, 0, None); refused("ops[3].kind", ops)
    ops = base(); ops[2] = point(P.TOP_APPEND_POINT); refused("ops[3].kind", ops)
    ops = base(); ops[3] = T(P.TOP_RNG_BEGIN, None, 0, None, 0, 0, None); refused("ops[4].kind", ops)
    for kind in (P.TOP_RNG_FILL, P.TOP_RNG_FILL32, P.TOP_RNG_SCALARS):
        ops = base(); ops[0] = T(kind, None, 0, out2.data_ptr(), 64, 64, None); refused("ops[0].kind", ops, n_ops=1)
    # labels
    ops = base(); ops[1].label_len = 65; refused("ops[1].label_len", ops)
    for j in (2, 3, 4):
        ops = base(); ops[j].label, ops[j].label_len = lab, 1; refused("ops[%d].label" % j, ops)
    ops = base(); ops[3].kind = P.TOP_RNG_FILL; ops[3].label, ops[3].label_len = lab, 1; refused("ops[3].label", ops)
    # pointer kinds of the new operations' arrays
    for j in (1, 2, 3, 4):
        ops = base(); ops[j].data_dev = host.ctypes.data; refused("ops[%d].data_dev" % j, ops)
    ops = base(); ops[1].lens_dev = host.ctypes.data; refused("ops[1].lens_dev", ops)
    for kind in (P.TOP_APPEND_POINT, P.TOP_CHALLENGE_SCALAR):
        ops = base(); ops[4] = point(kind); ops[4].data_dev = host.ctypes.data; refused("ops[4].data_dev", ops)
    # an output range overlapping the states, an input, or another output
    ops = base(); ops[3].data_dev = states.data_ptr() + 203; refused("overlap", ops)
    ops = base(); ops[4].data_dev = wit.data_ptr() + 8; refused("overlap", ops)
    ops = base(); ops[4].data_dev = ent.data_ptr(); refused("overlap", ops)
    ops = base(); ops[4].data_dev = out.data_ptr() + 32; refused("overlap", ops)
    ops = base(); ops[4] = point(P.TOP_CHALLENGE_SCALAR, out); refused("overlap", ops)
    ops = base(); ops[4] = point(P.TOP_APPEND_POINT, out); refused("overlap", ops)
    assert packed.transcripts_stats(engine) == before
    # accepted: NullRng, a FILL of any length, two reads of the same rows
    ops = base(); ops[2] = T(P.TOP_RNG_FINALIZE, None, 0, None, 0, 0, None); accepted(ops)
    ops = base(); ops[3].kind, ops[3].len = P.TOP_RNG_FILL, 48; accepted(ops)
    ops = base(); ops[4] = point(P.TOP_APPEND_POINT, ent); accepted(ops)
    torch.cuda.synchronize()
    with pytest.raises(importlib.import_module("bulletproofs-plus_amd").ProofError) as e:
        packed.transcript_ops(engine, states, [packed.TRngBegin(), packed.TRngFill(64, out)])
    assert "finalised RNG" in str(e.value)


# ---------------------------------------------------------------- 8. steady state
def test_steady_state_allocates_nothing_and_waits_for_nothing(bpp, packed):
    eng = bpp.Engine(0)
    try:
        n = 64
        makers = [TC.at(k, (5 * k) % 166) for k in range(n)]
        prog = [("begin",), ("rekey", b"w", TC.messages(800, n, [32] * n)), ("finalize", TC.messages(801, n, [32] * n)), ("fill32", 64),
                ("scalars", 2)]
        want = TC.oracle_rows(makers, prog)
        ops = _ops(packed, prog, n)
        states = _dev(_states(makers))
        done, rec = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        last = None
        for _ in range(20):
            last = packed.transcript_ops(eng, states, ops, done_mask=done, record=rec)
        assert packed.transcripts_stats(eng) == {"calls": 20, "first_calls": 1, "host_waits": 0}
        assert last.result() == {"n_done": n, "n_void": 0, "first_void": None, "flags": WRITTEN}
        assert last.done()
        _hold(last, want, "the twentieth call")  # (no RNG operation changes a row: every call computed the same bytes)
    finally:
        eng.close()


# ---------------------------------------------------------------- 9. the loop closed
def test_the_loop_closed_rng_rows_and_blindings_made_on_the_device(bpp, packed):
    """NEW + APPEND(txid) make the rows; RNG_BEGIN / RNG_REKEY(secret) / RNG_FINALIZE(entropy) / RNG_FILL32 make the prover's rng rows
    and RNG_SCALARS the blinding factors, all on the device; ProvePlan.enqueue proves from them; the proofs equal the oracle's prover
    fed the oracle's own bytes for the same rows, and the verifier accepts them.  n = 3 items of m = 1 at 8 bits, as the loop of
    tests/test_gpu_transcript_ops.py."""
    n_bits, m_max, t, n = 8, 1, 1, 3
    rounds = (n_bits * 1).bit_length() - 1
    rng_len = 32 * (rounds + 3)
    rng = np.random.default_rng(9)
    values = rng.integers(0, 2 ** n_bits, size=(n, m_max)).astype(np.int64)
    txid, secret, entropy = (TC.messages(900 + k, n, [32] * n) for k in range(3))
    prog = [("append", b"txid", txid), ("begin",), ("rekey", b"secret", secret), ("finalize", entropy), ("fill32", rng_len), ("scalars", 1)]
    makers = [(lambda: M.Transcript(b"loop"))] * n
    o_states, o_outs, o_void = TC.oracle_rows(makers, prog)
    assert not any(o_void)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        eng = bpp.Engine(0, stream=stream.cuda_stream)
        params = bpp.RangeParameters.init(n_bits, m_max, bpp.create_pedersen_gens_with_extension_degree(t), engine=eng)
        plan = None
        try:
            states = torch.full((n, 203), 0xFF, dtype=torch.uint8, device="cuda")
            ext = torch.full((n, rng_len), 0xFF, dtype=torch.uint8, device="cuda")
            blind = torch.full((n, m_max, t, 32), 0xFF, dtype=torch.uint8, device="cuda")
            ops = _ops(packed, prog, n, new=b"loop")
            ops[5] = packed.TRngFill32(rng_len, ext)
            ops[6] = packed.TRngScalars(1, blind.view(n, 32))
            ms = np.ones(n, dtype=np.uint32)
            plan = packed.ProvePlan(eng, params, ms, m_stride=m_max, rng_stride=rng_len, item_states=True)
            openings = packed.DeviceOpenings(_dev(values), blind, ms, rng_bytes=ext, item_states=states)
            made = packed.transcript_ops(eng, states, ops)
            proved = plan.enqueue(openings, states=True)
            proved.wait()
            assert made.done() and made.result() == {"n_done": n, "n_void": 0, "first_void": None, "flags": WRITTEN}
            assert proved.result()["n_ok"] == n
            assert [bytes(r) for r in ext.cpu().numpy()] == o_outs[0] and [bytes(r) for r in blind.view(n, 32).cpu().numpy()] == o_outs[1]
            o_params = O.RangeParameters(n_bits, m_max, O.PedersenGens(t))
            proofs, commits = proved.proofs.cpu().numpy(), proved.commitments.cpu().numpy()
            for i in range(n):
                tr = M.Transcript(b"loop")
                tr.append_message(b"txid", txid[i])
                assert tr.strobe.to_bytes() == o_states[i]
                opening = O.CommitmentOpening(int(values[i, 0]), [int.from_bytes(o_outs[1][i], "little")])
                comm = o_params.pc_gens.commit(opening.v, opening.r)
                proof = O.prove_with_rng(tr, O.RangeStatement(o_params, [comm], [None], None), O.RangeWitness([opening]), M.ByteStreamRng(o_outs[0][i]))
                assert bytes(commits[i].reshape(-1)[:32]) == comm.compress(), "item %d: the commitment differs from the oracle's" % i
                assert bytes(proofs[i, :int(plan.proof_lens[i])]) == proof.to_bytes(), "item %d: the proof differs from the oracle's" % i
            masks, present = packed.verify_batch_mixed_device(params, proved.as_mixed_input())
            assert not present.any()
        finally:
            if plan is not None:
                plan.close()
            params.close()
            eng.close()
