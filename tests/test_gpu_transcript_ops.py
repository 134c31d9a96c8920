"""GPU tests of Merlin on the stream (bpp_transcripts_enqueue / packed.transcript_ops): Transcript::new, append_message and
challenge_bytes, row-wise, on transcript rows of 203 bytes in device memory.

Every expected byte comes from oracle.pyref.merlin.Transcript: a row is described by a function that makes its oracle transcript, the
program is applied to that object, and the 203 bytes and the challenge bytes it gives are compared with the device's, row by row.
The sizes are the smallest at which the kernel can go wrong: every starting position of the 166-byte block, message and challenge
lengths on either side of the rate, labels of 0 and 64 bytes, rows at odd addresses, one row and either side of a wavefront's worth."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from oracle.pyref import curve as C
from oracle.pyref import merlin as M
from oracle.pyref import protocol as O
from tests import transcript_sweep as TS

pytestmark = pytest.mark.gpu

RATE = 166
INVALID_ARGUMENT = 2
NONE = 0xFFFFFFFF
WRITTEN = 1
L64 = bytes((3 * i + 1) & 0xFF for i in range(64))


@pytest.fixture(scope="module")
def packed():
    return importlib.import_module("bulletproofs-plus_amd.packed")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _at(i, pos):
    """-> a function that makes row i's oracle transcript: a label of its own, one message whose length puts the sponge at `pos`"""
    def make(length=None):
        tr = M.Transcript(b"row %d" % i)
        if length is None:
            length = (pos - make(0).strobe.pos) % RATE
        tr.append_message(b"pad", bytes([i & 255]) * length)
        return tr
    assert make().strobe.pos == pos
    return make


def _states(makers):
    return np.stack([np.frombuffer(mk().strobe.to_bytes(), dtype=np.uint8) for mk in makers]).copy()


def _messages(seed, n, lengths):
    rng = np.random.default_rng(seed)
    return [bytes(rng.integers(0, 256, size=lengths[i], dtype=np.uint8)) for i in range(n)]


def _expect(makers, prog, new=None):
    """the oracle: prog = [("append", label, [message of row i]) | ("challenge", label, nbytes)] on every row's transcript ->
    (states uint8 [n, 203], [uint8 [n, nbytes] per challenge])"""
    states, outs = [], [[] for op in prog if op[0] == "challenge"]
    for i, mk in enumerate(makers):
        tr = M.Transcript(new) if new is not None else mk()
        c = 0
        for kind, label, x in prog:
            if kind == "append":
                tr.append_message(label, x[i])
            else:
                outs[c].append(np.frombuffer(tr.challenge_bytes(label, x), dtype=np.uint8))
                c += 1
        states.append(np.frombuffer(tr.strobe.to_bytes(), dtype=np.uint8))
    return np.stack(states), [np.stack(o) if o and o[0].size else np.zeros((len(makers), 0), dtype=np.uint8) for o in outs]


def _ops(packed, prog, n, lens=False, cap=None, new=None):
    """the device form of prog -> (ops, [the backing tensor of every op's rows])"""
    ops, backing = ([packed.TNew(new)] if new is not None else []), []
    for kind, label, x in prog:
        if kind == "append":
            width = cap if cap is not None else max(len(b) for b in x)
            assert lens or all(len(b) == width for b in x)
            arr = np.full((n, width), 0xEE, dtype=np.uint8)
            for i, b in enumerate(x):
                arr[i, :len(b)] = np.frombuffer(b, dtype=np.uint8)
            ten = _dev(arr) if width else None
            ops.append(packed.TAppend(label, ten, _dev(np.array([len(b) for b in x], dtype=np.int32)) if lens else None))
        else:
            ten = torch.full((n, x), 0xFF, dtype=torch.uint8, device="cuda") if x else None
            ops.append(packed.TChallenge(label, x, ten))
        backing.append(ten)
    return ops, backing


def _hold(res, want_states, want_outs, what=""):
    res.wait()
    got = res.states.cpu().numpy() if hasattr(res.states, "cpu") else None
    if got is not None:
        bad = [i for i in range(len(want_states)) if not np.array_equal(got[i], want_states[i])]
        assert not bad, "%s: state rows %s differ from the oracle's Merlin" % (what, bad[:8])
    for c, want in enumerate(want_outs):
        if want.shape[1] == 0:
            continue
        out = res.outputs[c].cpu().numpy()
        bad = [i for i in range(len(want)) if not np.array_equal(out[i], want[i])]
        assert not bad, "%s: challenge %d differs from the oracle's in rows %s" % (what, c, bad[:8])


# ---------------------------------------------------------------- 1. every starting position
def test_every_starting_position(engine, packed):
    lengths = list(range(RATE)) + [166, 167, 400]
    makers = [(lambda k=k: M.Transcript(TS.label_of(k))) for k in lengths]
    n = len(makers)
    assert n == 169 and sorted({mk().strobe.pos for mk in makers}) == list(range(RATE))
    prog = [("append", b"ctx", _messages(1, n, [40] * n)), ("challenge", b"c", 32), ("append", b"", _messages(2, n, [40] * n)),
            ("challenge", b"after", 64)]
    want_states, want_outs = _expect(makers, prog)
    ops, _ = _ops(packed, prog, n)
    res = packed.transcript_ops(engine, _dev(_states(makers)), ops)
    _hold(res, want_states, want_outs, "169 rows")
    assert res.done_mask.cpu().numpy().all()
    assert res.result() == {"n_done": n, "n_void": 0, "first_void": None, "flags": WRITTEN}


# ---------------------------------------------------------------- 2. either side of the rate
EDGE = [_at(k, (0, 1, 164, 165)[k % 4]) for k in range(12)]
EDGE_LENS = (0, 1, 165, 166, 167, 400)


@pytest.mark.parametrize("label", [b"", L64], ids=["label0", "label64"])
def test_uniform_lengths_either_side_of_the_rate(engine, packed, label):
    n = len(EDGE)
    for length in EDGE_LENS:
        prog = [("append", label, _messages(length, n, [length] * n)), ("challenge", label, 32)]
        want_states, want_outs = _expect(EDGE, prog)
        ops, _ = _ops(packed, prog, n)
        _hold(packed.transcript_ops(engine, _dev(_states(EDGE)), ops), want_states, want_outs, "len %d" % length)


def test_per_row_lengths_under_a_cap(engine, packed):
    n = len(EDGE)
    for shift in range(6):
        lengths = [EDGE_LENS[(k // 4 + k + shift) % 6] for k in range(n)]
        prog = [("append", b"ctx", _messages(10 + shift, n, lengths)), ("challenge", L64, 32), ("append", L64, _messages(20 + shift, n, lengths))]
        want_states, want_outs = _expect(EDGE, prog)
        ops, _ = _ops(packed, prog, n, lens=True, cap=400)
        res = packed.transcript_ops(engine, _dev(_states(EDGE)), ops)
        _hold(res, want_states, want_outs, "lens %s" % lengths)
        assert res.result()["n_done"] == n


@pytest.mark.parametrize("nbytes", [1, 32, 64, 200, 700])
def test_challenge_lengths(engine, packed, nbytes):
    """(700: more than two pieces of the kernel's 256-byte LDS buffer, and more than four blocks of the sponge)"""
    n = len(EDGE)
    for label in (b"", L64):
        prog = [("challenge", label, nbytes), ("append", b"x", _messages(3, n, [1] * n)), ("challenge", label, nbytes)]
        want_states, want_outs = _expect(EDGE, prog)
        ops, _ = _ops(packed, prog, n)
        _hold(packed.transcript_ops(engine, _dev(_states(EDGE)), ops), want_states, want_outs, "challenge of %d" % nbytes)


# ---------------------------------------------------------------- 3. NEW
@pytest.mark.parametrize("length", [0, 17, 165, 166, 400])
def test_new_then_append_and_challenge(engine, packed, length):
    n = 5
    label = TS.label_of(length)
    prog = [("append", b"txid", _messages(30 + length, n, [32] * n)), ("challenge", b"c", 32)]
    want_states, want_outs = _expect([None] * n, prog, new=label)
    ops, _ = _ops(packed, prog, n, new=label)
    states = torch.full((n, 203), 0xFF, dtype=torch.uint8, device="cuda")
    res = packed.transcript_ops(engine, states, ops)
    _hold(res, want_states, want_outs, "NEW with a label of %d bytes" % length)
    assert res.result()["n_done"] == n
    # NEW alone: bpp_transcript_new's bytes in every row
    only = packed.transcript_ops(engine, torch.full((n, 203), 0xFF, dtype=torch.uint8, device="cuda"), [packed.TNew(label)])
    only.wait()
    assert all(bytes(r) == M.Transcript(label).strobe.to_bytes() for r in only.states.cpu().numpy())


# ---------------------------------------------------------------- 4. void and dead rows
def _void_case():
    """nine rows: dead, valid, zeros, pos 166, dead, pos 255, valid with lens = len + 1, valid, dead"""
    makers = [_at(k, (0, 1, 2, 3, 164, 5, 165, 83, 7)[k]) for k in range(9)]
    rows = _states(makers)
    rows[2] = 0
    rows[3] = 0xFF
    rows[3, 200], rows[3, 202] = 166, 2
    rows[5] = 0xFF
    rows[5, 200], rows[5, 202] = 255, 2
    live = np.array([0, 1, 1, 1, 0, 1, 1, 1, 0], dtype=np.uint8)
    lengths = [24] * 9
    lengths[6] = 41
    return makers, rows, live, lengths


def test_void_and_dead_rows(engine, packed):
    makers, rows, live, lengths = _void_case()
    n, cap = 9, 40
    msgs = _messages(40, n, [24] * n)
    prog = [("append", b"ctx", msgs), ("challenge", b"c", 32), ("append", b"tail", _messages(41, n, [8] * n))]
    want_states, want_outs = _expect(makers, prog)
    ops, _ = _ops(packed, prog, n)
    # the first append under a cap, row 6 with a length beyond it
    data = np.full((n, cap), 0xFF, dtype=np.uint8)
    for i in range(n):
        data[i, :24] = np.frombuffer(msgs[i], dtype=np.uint8)
    ops[0] = packed.TAppend(b"ctx", _dev(data), _dev(np.array(lengths, dtype=np.int32)))
    states = _dev(rows)
    res = packed.transcript_ops(engine, states, ops, live=_dev(live))
    res.wait()
    got, out = res.states.cpu().numpy(), res.outputs[0].cpu().numpy()
    dead, void, valid = [0, 4, 8], [2, 3, 5, 6], [1, 7]
    for i in dead:
        assert np.array_equal(got[i], rows[i]), "dead row %d was written" % i
        assert not out[i].any(), "dead row %d: its challenge row is not zero" % i
    for i in void:
        assert not got[i].any() and not out[i].any(), "void row %d is not zero" % i
    for i in valid:
        assert np.array_equal(got[i], want_states[i]) and np.array_equal(out[i], want_outs[0][i]), "row %d differs from the oracle's" % i
    assert list(res.done_mask.cpu().numpy()) == [0, 1, 0, 0, 0, 0, 0, 1, 0]
    assert res.result() == {"n_done": 2, "n_void": 4, "first_void": 2, "flags": WRITTEN}


def test_all_dead_and_all_void(engine, packed):
    n = 5
    makers = [_at(k, k) for k in range(n)]
    rows = _states(makers)
    msgs = _messages(50, n, [40] * n)
    ops, _ = _ops(packed, [("append", b"ctx", msgs), ("challenge", b"c", 32)], n)
    res = packed.transcript_ops(engine, _dev(rows), ops, live=torch.zeros(n, dtype=torch.uint8, device="cuda"),
                                done_mask=torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda"))
    assert res.result() == {"n_done": 0, "n_void": 0, "first_void": None, "flags": WRITTEN}
    assert np.array_equal(res.states.cpu().numpy(), rows) and not res.outputs[0].cpu().numpy().any() and not res.done_mask.cpu().numpy().any()
    ops, _ = _ops(packed, [("append", b"ctx", msgs), ("challenge", b"c", 32)], n)
    res = packed.transcript_ops(engine, torch.zeros((n, 203), dtype=torch.uint8, device="cuda"), ops,
                                done_mask=torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda"))
    assert res.result() == {"n_done": 0, "n_void": n, "first_void": 0, "flags": WRITTEN}
    assert not res.states.cpu().numpy().any() and not res.outputs[0].cpu().numpy().any() and not res.done_mask.cpu().numpy().any()


# ---------------------------------------------------------------- 5. geometry
@pytest.mark.parametrize("n", [1, 63, 64, 65])
@pytest.mark.parametrize("offset", [1, 3])
def test_rows_at_odd_addresses_with_slack(engine, packed, n, offset):
    makers = [_at(k, (37 * k) % RATE) for k in range(n)]
    rows = _states(makers)
    msgs = _messages(60 + n, n, [32] * n)
    want_states, want_outs = _expect(makers, [("append", b"txid", msgs), ("challenge", b"c", 32)])
    sbuf = torch.full((offset + n * 203 + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    sbuf[offset:offset + n * 203] = _dev(rows).reshape(-1)
    states = sbuf[offset:offset + n * 203].view(n, 203)
    assert states.data_ptr() % 4 == offset
    data = np.full((n, 33), 0xEE, dtype=np.uint8)
    for i in range(n):
        data[i, :32] = np.frombuffer(msgs[i], dtype=np.uint8)
    dbuf = torch.full((1 + n * 33 + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    dbuf[1:1 + n * 33] = _dev(data).reshape(-1)
    obuf = torch.full((1 + n * 33 + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    rows33 = lambda buf: buf[1:1 + n * 33].view(n, 33)[:, :32]  # noqa: E731
    assert rows33(dbuf).data_ptr() % 2 == 1 and rows33(obuf).data_ptr() % 2 == 1
    # (a view of one row has no stride to read: the tuple form names it)
    pair = lambda buf: (rows33(buf).data_ptr(), (n, 32), 33)  # noqa: E731
    torch.cuda.synchronize()
    res = packed.transcript_ops(engine, states, [packed.TAppend(b"txid", pair(dbuf)), packed.TChallenge(b"c", 32, pair(obuf))])
    res.wait()
    s, o, d = sbuf.cpu().numpy(), obuf.cpu().numpy(), dbuf.cpu().numpy()
    assert np.array_equal(s[offset:offset + n * 203].reshape(n, 203), want_states)
    assert (s[:offset] == 0xEE).all() and (s[offset + n * 203:] == 0xEE).all(), "a byte outside the rows was written"
    got = o[1:1 + n * 33].reshape(n, 33)
    assert np.array_equal(got[:, :32], want_outs[0])
    assert (got[:, 32] == 0xEE).all() and o[0] == 0xEE and (o[1 + n * 33:] == 0xEE).all(), "row slack of the challenge was written"
    assert np.array_equal(d[1:1 + n * 33].reshape(n, 33), data) and d[0] == 0xEE
    assert res.result()["n_done"] == n


# ---------------------------------------------------------------- 6. refusals
def test_refusals_before_any_launch(engine, packed):
    lib, T = engine.lib, packed._lib.TranscriptOp
    n = 4
    states = torch.zeros((n, 203), dtype=torch.uint8, device="cuda")
    data = torch.zeros((n, 40), dtype=torch.uint8, device="cuda")
    out = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    lens = torch.zeros((n,), dtype=torch.int32, device="cuda")
    live = torch.ones((n,), dtype=torch.uint8, device="cuda")
    done = torch.zeros((n,), dtype=torch.uint8, device="cuda")
    rec = torch.zeros((4,), dtype=torch.int32, device="cuda")
    label = (ctypes.c_uint8 * 400)()
    lab = ctypes.addressof(label)
    host = np.zeros(4096, dtype=np.uint8)  # host memory: never dereferenced

    def base():
        ops = (T * 9)()
        ops[0] = T(packed.TOP_APPEND, lab, 3, data.data_ptr(), 40, 40, lens.data_ptr())
        ops[1] = T(packed.TOP_CHALLENGE, lab, 1, out.data_ptr(), 32, 32, None)
        return ops

    def call(ops, nn=n, n_ops=2, st=None, lv=None, dn=None, rc_=None):
        addr = lambda a, d: ctypes.c_void_p(d.data_ptr() if a is None else int(a))  # noqa: E731
        rc = lib.bpp_transcripts_enqueue(engine.ctx, addr(st, states), nn, ops, n_ops, addr(lv, live), addr(dn, done), addr(rc_, rec), None)
        return rc, lib.bpp_ctx_last_error(engine.ctx).decode()

    def refused(needle, *a, **kw):
        rc, msg = call(*a, **kw)
        assert rc == INVALID_ARGUMENT and needle in msg, (needle, rc, msg)

    torch.cuda.synchronize()
    assert call(base())[0] == 0
    before = packed.transcripts_stats(engine)
    refused("n is 0", base(), nn=0)
    refused("n_ops", base(), n_ops=0)
    refused("n_ops", base(), n_ops=9)
    ops = base(); ops[1].kind = 7; refused("ops[1].kind", ops)
    ops = base(); ops[1] = T(packed.TOP_NEW, lab, 3, None, 0, 0, None); refused("NEW must be op 0", ops)
    ops = base(); ops[0] = T(packed.TOP_NEW, lab, 3, data.data_ptr(), 0, 0, None); refused("NEW takes no data", ops)
    ops = base(); ops[0].label_len = 65; refused("ops[0].label_len", ops)
    ops = base(); ops[1].len, ops[1].stride = 65537, 65537; refused("ops[1].len", ops)
    ops = base(); ops[1].stride = 31; refused("ops[1].stride", ops)
    ops = base(); ops[0].data_dev = None; refused("ops[0].data_dev", ops)
    ops = base(); ops[1].lens_dev = lens.data_ptr(); refused("ops[1].lens_dev", ops)
    # pointers bpp_device_pointer_check does not class as this device's memory
    refused("states203_dev", base(), st=host.ctypes.data)
    ops = base(); ops[0].data_dev = host.ctypes.data; refused("ops[0].data_dev", ops)
    ops = base(); ops[1].data_dev = host.ctypes.data; refused("ops[1].data_dev", ops)
    ops = base(); ops[0].lens_dev = host.ctypes.data; refused("ops[0].lens_dev", ops)
    refused("live_dev", base(), lv=host.ctypes.data)
    refused("done_mask_dev", base(), dn=host.ctypes.data)
    refused("record_dev", base(), rc_=host.ctypes.data)
    # a written range that overlaps another range of the call
    ops = base(); ops[1].data_dev = states.data_ptr() + 203 * 3; refused("overlap", ops)
    ops = base(); ops[1].data_dev = data.data_ptr() + 8; refused("overlap", ops)
    refused("overlap", base(), dn=states.data_ptr() + 100)
    refused("overlap", base(), rc_=done.data_ptr())
    refused("overlap", base(), lv=states.data_ptr())
    assert packed.transcripts_stats(engine) == before
    # NEW's label may have any length; a long one is no refusal
    ops = base(); ops[0] = T(packed.TOP_NEW, lab, 400, None, 0, 0, None)
    assert call(ops)[0] == 0
    torch.cuda.synchronize()
    # ... and the wrapper raises with the engine's words
    with pytest.raises(importlib.import_module("bulletproofs-plus_amd").ProofError) as e:
        packed.transcript_ops(engine, states, [packed.TChallenge(b"c", 32, out), packed.TNew(b"late")])
    assert "NEW must be op 0" in str(e.value)


# ---------------------------------------------------------------- 7. steady state
def test_steady_state_allocates_nothing_and_waits_for_nothing(bpp, packed):
    eng = bpp.Engine(0)
    try:
        n = 64
        makers = [_at(k, (5 * k) % RATE) for k in range(n)]
        prog = [("append", b"ctx", _messages(70, n, [32] * n)), ("challenge", b"c", 32)]
        ops, _ = _ops(packed, prog, n)
        states = _dev(_states(makers))
        done, rec = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        last = None
        for _ in range(20):
            last = packed.transcript_ops(eng, states, ops, done_mask=done, record=rec)
        assert packed.transcripts_stats(eng) == {"calls": 20, "first_calls": 1, "host_waits": 0}
        assert last.result() == {"n_done": n, "n_void": 0, "first_void": None, "flags": WRITTEN}
        assert last.done()
    finally:
        eng.close()


# ---------------------------------------------------------------- 8. the loop
def test_the_loop_rows_made_and_continued_on_the_stream(bpp, packed):
    """rows made on the device (NEW + APPEND of a transaction id each) -> prove -> refill -> verify -> CHALLENGE on the rows the
    verifier hands back: one stream, one wait.  One proof has a bit flipped on the device between prove and refill: its group is
    rejected, its row comes back zero, and the call leaves it void with a zero challenge."""
    n_bits, m_max, t, ms = 8, 4, 1, [1, 2, 1, 4]
    n, spoiled = len(ms), 2
    rounds = lambda m: (n_bits * m).bit_length() - 1  # noqa: E731
    rng = np.random.default_rng(8)
    values = np.zeros((n, m_max), dtype=np.int64)
    blind = np.zeros((n, m_max, t, 32), dtype=np.uint8)
    ext = np.zeros((n, 32 * (rounds(m_max) + 3)), dtype=np.uint8)
    for i, m in enumerate(ms):
        values[i, :m] = rng.integers(0, 2 ** n_bits, size=m)
        blind[i, :m] = rng.integers(0, 256, size=(m, t, 32), dtype=np.uint8)
        blind[i, :m, :, 31] &= 0x0F
        ext[i, :32 * (rounds(m) + 3)] = rng.integers(0, 256, size=32 * (rounds(m) + 3), dtype=np.uint8)
    txid = [rng.integers(0, 256, size=(n, 32), dtype=np.uint8) for _ in range(2)]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        eng = bpp.Engine(0, stream=stream.cuda_stream)
        params = bpp.RangeParameters.init(n_bits, m_max, bpp.create_pedersen_gens_with_extension_degree(t), engine=eng)
        plan = rb = None
        try:
            states = torch.full((n, 203), 0xFF, dtype=torch.uint8, device="cuda")
            txid_dev = _dev(txid[0])
            make = [packed.TNew(b"loop"), packed.TAppend(b"txid", txid_dev)]
            plan = packed.ProvePlan(eng, params, np.array(ms, dtype=np.uint32), m_stride=m_max, rng_stride=ext.shape[1], item_states=True)
            openings = packed.DeviceOpenings(_dev(values), _dev(blind), np.array(ms, dtype=np.uint32), rng_bytes=_dev(ext), item_states=states)
            nxt_out = torch.full((n, 32), 0xFF, dtype=torch.uint8, device="cuda")
            # a first step with the first transaction ids: the plan's first call, the batch, its layout and its first refill
            packed.transcript_ops(eng, states, make)
            warm = plan.enqueue(openings, states=True)
            rb = packed.ResidentBatch.from_mixed(params, warm.as_mixed_input())
            rb.enqueue(chunk=1, states=True).wait()
            rb.refill(warm.as_mixed_input(), shape_vectors=False)
            warmed = rb.enqueue(chunk=1, states=True)
            packed.transcript_ops(eng, warmed.states, [packed.TChallenge(b"next", 32, nxt_out)]).wait()
            assert all(r["code"] == 0 for r in warmed.results())
            s0 = packed.transcripts_stats(eng)
            # ---- the step: no wait between the calls
            txid_dev.copy_(_dev(txid[1]))
            states.fill_(0xFF)
            made = packed.transcript_ops(eng, states, make)
            proved = plan.enqueue(openings, states=True)
            proved.proofs[spoiled, 1 + 32 * 4] ^= 1  # r1 of one proof, on the device, on the stream
            filled = rb.refill(proved.as_mixed_input(), shape_vectors=False)
            checked = rb.enqueue(chunk=1, states=True)
            nxt = packed.transcript_ops(eng, checked.states, [packed.TChallenge(b"next", 32, nxt_out)])
            s1 = packed.transcripts_stats(eng)
            nxt.wait()  # the one wait of the step
            assert s1["calls"] == s0["calls"] + 2 and s1["host_waits"] == s0["host_waits"] == 0 and s1["first_calls"] == s0["first_calls"] == 1
            assert made.done() and proved.done() and filled.done() and checked.done()
            codes = [r["code"] for r in checked.results()]
            assert [c == 0 for c in codes] == [i != spoiled for i in range(n)], codes
            assert proved.result()["n_ok"] == n and filled.result()["code"] == 0
            got_states, got_next = nxt.states.cpu().numpy(), nxt.outputs[0].cpu().numpy()
            assert not got_states[spoiled].any() and not got_next[spoiled].any()
            assert list(nxt.done_mask.cpu().numpy()) == [int(i != spoiled) for i in range(n)]
            assert nxt.result() == {"n_done": n - 1, "n_void": 1, "first_void": spoiled, "flags": WRITTEN}
            # the oracle: its own Merlin for the row, its verifier's appends on the device's proof, then the challenge
            o_params = O.RangeParameters(n_bits, m_max, O.PedersenGens(t))
            proofs, commits = proved.proofs.cpu().numpy(), proved.commitments.cpu().numpy()
            for i in range(n):
                if i == spoiled:
                    continue
                m = ms[i]
                tr = M.Transcript(b"loop")
                tr.append_message(b"txid", bytes(txid[1][i]))
                comms = [C.decompress(bytes(commits[i, 32 * j:32 * j + 32])) for j in range(m)]
                st = O.RangeStatement(o_params, comms, [None] * m, None)
                O.verify([tr], [st], [O.RangeProof.from_bytes(bytes(proofs[i, :int(plan.proof_lens[i])]))], 0)
                assert bytes(got_next[i]) == tr.challenge_bytes(b"next", 32), "item %d: the challenge differs from the oracle's" % i
                assert bytes(got_states[i]) == tr.strobe.to_bytes(), "item %d: the row differs from the oracle's" % i
        finally:
            if plan is not None:
                plan.close()
            if rb is not None:
                rb.close()
            params.close()
            eng.close()
