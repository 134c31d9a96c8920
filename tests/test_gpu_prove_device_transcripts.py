"""GPU tests of proving from device arrays with one transcript per item going in and the advanced transcripts coming out
(bpp_prove_openings_device_transcripts): the call writes what bpp_prove_openings_states writes on the equivalent bpp_prove_item array
whose item i has transcript_state = row i -- return code, message, per-item codes, lengths, proof and commitment bytes, zeroed slots
-- and row i of states_out is the transcript as challenge_final_e leaves it, or 203 zero bytes for an item that fails.

The reference of every comparison is bpp_prove_openings_states on the same engine; the oracle (oracle.pyref, whose prove_with_rng
advances its Transcript in place) is the reference for a few items besides.  The rows are Merlin transcripts built with the
oracle's Merlin: every row has a label of its own and one appended message whose length is chosen so that byte 200 (pos) takes each
of 0, 1, 83, 164 and 165 -- asserted where the rows are made -- so that the call-wide head crosses the rate boundary inside
different appends.  The host form leaves the state row of a failed item alone, the device form zeroes it: the host buffer is
prefilled with zeros, every other output with 0xA5 in both forms, and whole buffers are compared."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from oracle import cport
from oracle.pyref import curve as C
from oracle.pyref import merlin as M
from oracle.pyref import protocol as O
from tests.helpers import LABEL

pytestmark = pytest.mark.gpu

N, M_MAX, MS = 64, 8, 8
INVALID_ARGUMENT = 2
PATTERN = [1, 4, 2, 8, 1]
POSITIONS = [0, 1, 83, 164, 165]
RATE = 166
L_ORDER = 2 ** 252 + 27742317777372353535851937790883648493
TEXT = "transcript state has pos >= rate"
_CACHE = {}


def _params(bpp, engine, t):
    if t not in _CACHE:
        _CACHE[t] = bpp.RangeParameters.init(N, M_MAX, bpp.create_pedersen_gens_with_extension_degree(t), engine=engine)
    return _CACHE[t]


def _rounds(m):
    return (N * m).bit_length() - 1


def _plen(m, t):
    return 1 + 32 * (t + 5 + 2 * _rounds(m))


def _transcript(i, pos):
    """item i's transcript: a label of its own, one message; the message length puts the sponge at `pos`"""
    def make(length):
        tr = M.Transcript(b"session %d" % i)
        tr.append_message(b"ctx", bytes([i & 255]) * length)
        return tr
    length = (pos - make(0).strobe.pos) % RATE
    tr = make(length)
    assert tr.strobe.pos == pos, (i, pos, tr.strobe.pos)
    return tr


def _rows(n):
    """-> (uint8 [n, 203], the pos of every row): all distinct, the five positions in turn"""
    pos = [POSITIONS[i % 5] for i in range(n)]
    rows = np.stack([np.frombuffer(_transcript(i, p).strobe.to_bytes(), dtype=np.uint8) for i, p in enumerate(pos)])
    assert [int(r[200]) for r in rows] == pos and len({bytes(r) for r in rows}) == n
    return rows.copy(), pos


def _scalars(rng, shape):
    a = rng.integers(0, 256, size=tuple(shape) + (32,), dtype=np.uint8)
    a[..., 31] &= 0x0F  # < 2^252 < l
    return a


def _data(t, ms, seed):
    """the arrays of a call, rows of MS entries; slack holds what would be a finding if it were read"""
    rng = np.random.default_rng(seed)
    n = len(ms)
    d = dict(t=t, n=n, m=np.array(ms, dtype=np.uint32))
    d["values"] = np.full((n, MS), 2 ** 64 - 1, dtype=np.uint64)
    d["blind"] = np.full((n, MS, t, 32), 0xFF, dtype=np.uint8)
    d["minv"] = np.full((n, MS), 2 ** 64 - 1, dtype=np.uint64)
    d["minp"] = np.full((n, MS), 0xFF, dtype=np.uint8)
    d["rng"] = np.full((n, 32 * (_rounds(M_MAX) + 3) + 8), 0xFF, dtype=np.uint8)
    for i, m in enumerate(ms):
        if m not in (1, 2, 4, 8):
            continue
        d["values"][i, :m] = rng.integers(0, 2 ** (N - 1), size=m, dtype=np.uint64)
        d["blind"][i, :m] = _scalars(rng, (m, t))
        d["minp"][i, :m] = [(i + j) % 2 == 0 for j in range(m)]
        d["minv"][i, :m] = d["values"][i, :m] // 3
        need = 32 * (_rounds(m) + 3)
        d["rng"][i, :need] = rng.integers(0, 256, size=need, dtype=np.uint8)
    return d


def _host(engine, params, packed, d, rows, ps, cs, label=None, state=None):
    """bpp_prove_openings_states on the equivalent items (transcript_state = row i; rows None: the call's label or state) ->
    dict(rc, msg, codes, lens, proofs, commits, states, texts).  The state buffer starts out zero: the host form leaves a failed
    item's row alone."""
    n = d["n"]
    keep = {k: np.ascontiguousarray(d[k]) for k in ("values", "blind", "minv", "minp", "rng")}
    items = np.zeros(n, dtype=packed._PROVE_ITEM)
    items["values"] = packed._rows(keep["values"])
    items["blindings32"] = packed._rows(keep["blind"])
    items["m"] = d["m"]
    items["min_values"] = packed._rows(keep["minv"])
    items["min_present"] = packed._rows(keep["minp"])
    if rows is not None:
        keep["rows"] = np.ascontiguousarray(rows)
        items["transcript_state"] = packed._rows(keep["rows"])
    elif state is not None:
        keep["state"] = np.frombuffer(state, dtype=np.uint8).copy()
        items["transcript_state"] = keep["state"].ctypes.data
    else:
        keep["label"] = np.frombuffer(label, dtype=np.uint8).copy()
        items["transcript_label"] = keep["label"].ctypes.data
        items["label_len"] = len(label)
    items["rng_bytes"] = packed._rows(keep["rng"])
    items["rng_len"] = keep["rng"].shape[1]
    proofs = np.full((n, ps), 0xA5, dtype=np.uint8)
    commits = np.full((n, cs), 0xA5, dtype=np.uint8)
    states = np.zeros((n, 203), dtype=np.uint8)
    lens = np.zeros(n, dtype=np.uintp)
    codes = np.zeros(n, dtype=np.intc)
    err = ctypes.create_string_buffer(256)
    arr = items.ctypes.data_as(ctypes.POINTER(packed._lib.ProveItem))
    rc = engine.lib.bpp_prove_openings_states(engine.ctx, params.handle, arr, n, commits.ctypes.data, cs, proofs.ctypes.data, ps,
                                              lens.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t)),
                                              codes.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), states.ctypes.data, err, 256)
    texts = []
    for i in range(n):
        buf = ctypes.create_string_buffer(256)
        engine.lib.bpp_prove_openings_item_message(engine.ctx, params.handle, ctypes.byref(arr[i]), None, cs, ps, int(codes[i]), buf, 256)
        texts.append(buf.value.decode())
    return dict(rc=rc, msg=err.value.decode(), codes=codes, lens=lens, proofs=proofs, commits=commits, states=states, texts=texts)


def _dev(a):
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _openings(packed, d, rows, label=b"", state=None):
    return packed.DeviceOpenings(_dev(d["values"]), _dev(d["blind"]), d["m"], min_values=_dev(d["minv"]), min_present=_dev(d["minp"]),
                                 rng_bytes=_dev(d["rng"]), label=label, state=state, item_states=None if rows is None else _dev(rows))


def _device(params, packed, d, rows, ps, cs, states=True, label=b"", state=None):
    inp = _openings(packed, d, rows, label, state)
    proofs = torch.full((d["n"], ps), 0xA5, dtype=torch.uint8, device="cuda")
    commits = torch.full((d["n"], cs), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.full((d["n"], 203), 0xA5, dtype=torch.uint8, device="cuda") if states else None
    torch.cuda.synchronize()
    return packed.prove_openings_device(params, inp, commitments_out=commits, proofs_out=proofs, states=out)


def _same(engine, res, ref, rows=True):
    """everything the contract names, whole buffers: slack included (rows=False: all but the output rows)"""
    assert res.rc == ref["rc"] and res.message == ref["msg"], (res.rc, res.message, ref["rc"], ref["msg"])
    assert list(res.codes) == list(ref["codes"])
    assert list(res.proof_lens) == list(ref["lens"])
    st = res.status.cpu().numpy()
    assert list(st[:, 0]) == list(ref["codes"])
    assert [m for _, m in res.messages(engine)] == ref["texts"]
    if not rows:
        return
    got_p, got_c, got_s = res.proofs.cpu().numpy(), res.commitments.cpu().numpy(), res.states.cpu().numpy()
    bad = [i for i in range(len(ref["codes"])) if not (np.array_equal(got_p[i], ref["proofs"][i]) and np.array_equal(got_c[i], ref["commits"][i]))]
    assert not bad, "rows %s differ from bpp_prove_openings_states on host copies of the same arrays" % bad[:8]
    bad = [i for i in range(len(ref["codes"])) if not np.array_equal(got_s[i], ref["states"][i])]
    assert not bad, "state rows %s differ from bpp_prove_openings_states" % bad[:8]


def _no_secrets_left(engine):
    examined, nonzero = ctypes.c_uint64(), ctypes.c_uint64()
    assert engine.lib.bpp_prove_secret_bytes(engine.ctx, ctypes.byref(examined), ctypes.byref(nonzero)) == 0
    assert examined.value > 0 and nonzero.value == 0


def _against_oracle(d, pos, proofs, commits, states, lens, which):
    """the oracle's prover under item i's transcript: commitments, proof bytes and the transcript it leaves"""
    t = d["t"]
    cp = cport.Params(N, M_MAX, t)
    op = O.RangeParameters(N, M_MAX, O.PedersenGens(t))
    for i in which:
        m = int(d["m"][i])
        vals = [int(v) for v in d["values"][i, :m]]
        blinds = [[bytes(d["blind"][i, j, k]) for k in range(t)] for j in range(m)]
        mins = [int(d["minv"][i, j]) if d["minp"][i, j] else None for j in range(m)]
        ext = bytes(d["rng"][i, :32 * (_rounds(m) + 3)])
        comms = [cp.commit(vals[j], blinds[j]) for j in range(m)]
        ost = O.RangeStatement(op, [C.decompress(c) for c in comms], mins, None)
        ow = O.RangeWitness([O.CommitmentOpening(vals[j], [int.from_bytes(x, "little") for x in blinds[j]]) for j in range(m)])
        tr = _transcript(i, pos[i])
        proof = O.prove_with_rng(tr, ost, ow, M.ByteStreamRng(ext)).to_bytes()
        assert bytes(commits[i, :32 * m]) == b"".join(bytes(c) for c in comms), "commitments of item %d differ from the oracle's" % i
        assert bytes(proofs[i, :int(lens[i])]) == proof, "proof %d differs from the oracle prover's under its own transcript" % i
        assert bytes(states[i]) == tr.strobe.to_bytes(), "advanced transcript %d differs from the oracle's" % i
    cp.close()


# ---------------------------------------------------------------- 1. one item
def test_one_item_rows_in_and_out(bpp, engine):
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    params = _params(bpp, engine, 1)
    d = _data(1, [1], 1)
    rows, pos = _rows(1)
    ps, cs = _plen(1, 1) + 7, 32 * MS
    res = _device(params, packed, d, rows, ps, cs)
    assert res.rc == 0, res.message
    _same(engine, res, _host(engine, params, packed, d, rows, ps, cs))
    _against_oracle(d, pos, res.proofs.cpu().numpy(), res.commitments.cpu().numpy(), res.states.cpu().numpy(), res.proof_lens, [0])


# ---------------------------------------------------------------- 2. five items at odd addresses, the five positions
def test_five_positions_at_odd_addresses(bpp, engine):
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    t = 3
    params = _params(bpp, engine, t)
    d = _data(t, PATTERN, 2)
    rows, pos = _rows(5)
    assert pos == POSITIONS
    ps, cs = _plen(8, t) + 7, 32 * MS + 1
    keep = []

    def odd(a, fill=None):
        """a copy of `a` (or `fill` bytes of 0xA5 ...) in device memory at an odd byte address -> (address, the backing tensor)"""
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1) if fill is None else np.full(fill, 0xA5, dtype=np.uint8)
        buf = torch.full((raw.size + 1 + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        buf[1:1 + raw.size] = torch.from_numpy(raw).cuda()
        keep.append(buf)
        assert (buf.data_ptr() + 1) % 2 == 1
        return buf.data_ptr() + 1, buf

    pair = lambda k: (odd(d[k])[0], d[k].shape)  # noqa: E731
    inp = packed.DeviceOpenings(pair("values"), pair("blind"), d["m"], min_values=pair("minv"), min_present=pair("minp"), rng_bytes=pair("rng"),
                                item_states=(odd(rows)[0], rows.shape))
    addr_p, buf_p = odd(None, 5 * ps)
    addr_c, buf_c = odd(None, 5 * cs)
    addr_s, buf_s = odd(None, 5 * 203)
    torch.cuda.synchronize()
    res = packed.prove_openings_device(params, inp, commitments_out=(addr_c, (5, cs)), proofs_out=(addr_p, (5, ps)), states=addr_s)
    assert res.rc == 0 and not any(res.codes), res.message
    ref = _host(engine, params, packed, d, rows, ps, cs)
    _same(engine, res, ref, rows=False)
    got_p = buf_p.cpu().numpy()[1:1 + 5 * ps].reshape(5, ps)
    got_c = buf_c.cpu().numpy()[1:1 + 5 * cs].reshape(5, cs)
    got_s = buf_s.cpu().numpy()[1:1 + 5 * 203].reshape(5, 203)
    assert np.array_equal(got_p, ref["proofs"]) and np.array_equal(got_c, ref["commits"]) and np.array_equal(got_s, ref["states"])
    for buf, used in ((buf_p, 5 * ps), (buf_c, 5 * cs), (buf_s, 5 * 203)):
        host = buf.cpu().numpy()
        assert host[0] == 0xA5 and (host[1 + used:] == 0xA5).all() and host[1 + used:].size == 16, "a byte outside the rows was written"
    _against_oracle(d, pos, got_p, got_c, got_s, res.proof_lens, [0, 3])
    _no_secrets_left(engine)


# ---------------------------------------------------------------- 3. two sub-batches, the device loop closed
def test_two_sub_batches_and_the_outputs_verify_under_their_own_transcripts(bpp, engine, opt):
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    t = 1
    params = _params(bpp, engine, t)
    ms = (PATTERN * 14)[:67]
    d = _data(t, ms, 3)
    rows, _ = _rows(67)
    ps, cs = _plen(8, t) + 7, 32 * MS
    ref = _host(engine, params, packed, d, rows, ps, cs)
    assert ref["rc"] == 0
    res = None
    for ct in (0, 1, 2):
        opt("ct", ct)
        res = _device(params, packed, d, rows, ps, cs)
        _same(engine, res, ref)
    opt("ct", -1)
    # the outputs verify where they lie, every one under the transcript it continued
    inp = res.as_mixed_input()
    assert inp.item_states is not None
    packed.verify_batch_mixed_device(params, inp)
    rb = packed.ResidentBatch.from_mixed(params, res.as_mixed_input())
    out = rb.enqueue(chunk=16, states=True)
    assert all(r["code"] == 0 for r in out.results())
    rb.close()
    # ... and under no other: the same outputs with the rows rotated by one item
    rotated = packed.DeviceMixedInput(res.proofs, res.proof_lens, res.m, res.commitments.view(67, -1, 32), min_values=_dev(d["minv"]),
                                      min_present=_dev(d["minp"]), item_states=_dev(np.roll(rows, 1, axis=0)))
    with pytest.raises(bpp.ProofError):
        packed.verify_batch_mixed_device(params, rotated)


# ---------------------------------------------------------------- 4. findings
def _bad_row(rows, i, pos):
    """row i with a bad pos; everything else of it holds 0xFF: nothing of it but byte 200 may matter"""
    rows[i] = 0xFF
    rows[i, 200] = pos


def _zero_slots(res, d, which):
    got_p, got_c, got_s = res.proofs.cpu().numpy(), res.commitments.cpu().numpy(), res.states.cpu().numpy()
    for i in which:
        used, m = int(res.proof_lens[i]), int(d["m"][i])
        assert not got_p[i, :used].any() and (got_p[i, used:] == 0xA5).all()
        assert not got_c[i, :32 * m].any() and (got_c[i, 32 * m:] == 0xA5).all()
        assert not got_s[i].any()


def test_a_bad_pos_is_the_items_finding(bpp, engine):
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    t = 1
    params = _params(bpp, engine, t)
    d = _data(t, PATTERN, 4)
    rows, _ = _rows(5)
    host_rows = rows.copy()
    for i in (0, 2, 4):
        host_rows[i, 200] = RATE
        _bad_row(rows, i, RATE)
    ps, cs = _plen(8, t) + 3, 32 * MS
    ref = _host(engine, params, packed, d, host_rows, ps, cs)
    assert [int(c) for c in ref["codes"]] == [INVALID_ARGUMENT, 0, INVALID_ARGUMENT, 0, INVALID_ARGUMENT] and ref["texts"][0] == TEXT
    before = packed.prove_device_stats(engine)
    res = _device(params, packed, d, rows, ps, cs)
    _same(engine, res, ref)
    assert res.rc == INVALID_ARGUMENT and res.message == TEXT
    _zero_slots(res, d, (0, 2, 4))
    assert [int(x) for x in res.status.cpu().numpy()[:, 1]] == [13, 0, 13, 0, 13]
    after = packed.prove_device_stats(engine)
    assert after["device_findings"] - before["device_findings"] == 3 and after["calls"] - before["calls"] == 1
    _no_secrets_left(engine)


def test_the_blinding_factor_comes_before_the_transcript(bpp, engine):
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    t = 3
    params = _params(bpp, engine, t)
    d = _data(t, PATTERN, 5)
    rows, _ = _rows(5)
    d["blind"][3, 7, t - 1] = np.frombuffer(L_ORDER.to_bytes(32, "little"), dtype=np.uint8)
    host_rows = rows.copy()
    host_rows[3, 200] = 200
    _bad_row(rows, 3, 200)
    ps, cs = _plen(8, t), 32 * MS
    ref = _host(engine, params, packed, d, host_rows, ps, cs)
    assert ref["texts"][3] == "blinding factor is not canonical" and sum(1 for c in ref["codes"] if c) == 1
    res = _device(params, packed, d, rows, ps, cs)
    _same(engine, res, ref)
    _zero_slots(res, d, (3,))


def test_every_row_bad(bpp, engine):
    """Codes, messages and lengths are the host form's; the rows are not compared with it (bpp_prove_openings_states returns before
    it zeroes anything when no item passes its host checks).  Asserted: every slot is zeroed, the return code is the first item's."""
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    t = 1
    params = _params(bpp, engine, t)
    d = _data(t, PATTERN, 6)
    rows, _ = _rows(5)
    host_rows = rows.copy()
    for i in range(5):
        host_rows[i, 200] = RATE + 17 * i
        _bad_row(rows, i, RATE + 17 * i)
    ps, cs = _plen(8, t), 32 * MS
    ref = _host(engine, params, packed, d, host_rows, ps, cs)
    assert all(c == INVALID_ARGUMENT for c in ref["codes"]) and ref["rc"] == INVALID_ARGUMENT
    res = _device(params, packed, d, rows, ps, cs)
    _same(engine, res, ref, rows=False)
    assert res.rc == ref["codes"][0] and res.message == TEXT
    _zero_slots(res, d, range(5))
    _no_secrets_left(engine)


def test_a_refused_item_beside_a_bad_row(bpp, engine):
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    t = 1
    params = _params(bpp, engine, t)
    ms = [1, 3, 4, 2, 8]
    d = _data(t, ms, 7)
    rows, _ = _rows(5)
    host_rows = rows.copy()
    host_rows[2, 200] = 255
    _bad_row(rows, 2, 255)
    rows[1] = 0xFF  # (the refused item's row is never read)
    ps, cs = _plen(8, t), 32 * MS
    ref = _host(engine, params, packed, d, host_rows, ps, cs)
    assert ref["texts"][1] == "Number of commitments must be a power of two" and ref["texts"][2] == TEXT
    assert [int(c != 0) for c in ref["codes"]] == [0, 1, 1, 0, 0]
    before = packed.prove_device_stats(engine)
    res = _device(params, packed, d, rows, ps, cs)
    _same(engine, res, ref)
    assert not res.states.cpu().numpy()[[1, 2]].any()
    after = packed.prove_device_stats(engine)
    assert after["host_findings"] - before["host_findings"] == 1 and after["device_findings"] - before["device_findings"] == 1
    # no item passes the host's checks: the state rows are zeroed all the same
    d3 = _data(t, [3, 0, 16], 8)
    res = _device(params, packed, d3, _rows(3)[0], ps, cs)
    assert all(res.codes) and not res.states.cpu().numpy().any()


# ---------------------------------------------------------------- 5. one transcript for the call, states out
@pytest.mark.parametrize("source", ["label", "state"])
def test_states_out_under_the_calls_one_transcript(bpp, engine, source):
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    t = 1
    params = _params(bpp, engine, t)
    d = _data(t, PATTERN, 9)
    state = _transcript(7, 83).strobe.to_bytes() if source == "state" else None
    ps, cs = _plen(8, t), 32 * MS
    ref = _host(engine, params, packed, d, None, ps, cs, label=LABEL, state=state)
    assert ref["rc"] == 0
    res = _device(params, packed, d, None, ps, cs, label=b"" if state else LABEL, state=state)
    _same(engine, res, ref)
    assert len({bytes(r) for r in res.states.cpu().numpy()}) == 5


# ---------------------------------------------------------------- 6. refusals before any launch
def test_refusals_before_any_launch(bpp, engine, opt):
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    t = 1
    params = _params(bpp, engine, t)
    d = _data(t, PATTERN, 10)
    rows, _ = _rows(5)
    ps, cs = _plen(8, t), 32 * MS
    assert _device(params, packed, d, rows, ps, cs).rc == 0  # (the arena exists from here on)
    before = packed.prove_device_stats(engine)
    dev_rows = _dev(rows)
    out = torch.zeros((5, 203), dtype=torch.uint8, device="cuda")

    def call(item_states, states, label=b"", state=None):
        inp = packed.DeviceOpenings(_dev(d["values"]), _dev(d["blind"]), d["m"], min_values=_dev(d["minv"]), min_present=_dev(d["minp"]),
                                    rng_bytes=_dev(d["rng"]), label=label, state=state, item_states=item_states)
        # (the mirror drops the call's transcript when rows are given; the engine's refusal needs the struct as it is)
        st = inp.struct if (label or state is not None) else inp.struct_without_transcript()
        proofs = torch.zeros((5, ps), dtype=torch.uint8, device="cuda")
        commits = torch.zeros((5, cs), dtype=torch.uint8, device="cuda")
        lens = np.zeros(5, dtype=np.uintp)
        err = ctypes.create_string_buffer(256)
        addr = lambda a: None if a is None else ctypes.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else int(a))  # noqa: E731
        rc = engine.lib.bpp_prove_openings_device_transcripts(engine.ctx, params.handle, ctypes.byref(st), inp.item_states, commits.data_ptr(), cs,
                                                              proofs.data_ptr(), ps, lens.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t)),
                                                              addr(states), None, None, err, 256)
        return rc, err.value.decode()

    def refused(needle, *a, **kw):
        rc, msg = call(*a, **kw)
        assert rc == INVALID_ARGUMENT and needle in msg, (rc, msg)

    refused("transcript_label", dev_rows, out, label=LABEL)
    refused("transcript_state", dev_rows, out, state=_transcript(1, 1).strobe.to_bytes())
    host_rows, host_out = rows.copy(), np.zeros((5, 203), dtype=np.uint8)
    refused("item_states_dev", (host_rows.ctypes.data, (5, 203)), out)
    refused("states_out_dev", dev_rows, host_out.ctypes.data)
    both = torch.zeros(2 * 5 * 203, dtype=torch.uint8, device="cuda")
    both[:5 * 203] = dev_rows.reshape(-1)
    refused("overlap", both[:5 * 203].view(5, 203), both.data_ptr() + 203 * 4)   # the last row in is the first row out
    refused("overlap", both[:5 * 203].view(5, 203), both.data_ptr())             # the same range
    refused("overlap", both[203:6 * 203].view(5, 203), both.data_ptr())          # the out rows end inside the in rows
    rc, msg = call(both[:5 * 203].view(5, 203), both.data_ptr() + 5 * 203)       # (end to end is no overlap)
    assert rc == 0, msg
    before["calls"] += 1
    before["items"] += 5
    opt("prove_check", 1)
    refused("prove_check", dev_rows, out)
    opt("prove_check", -1)
    assert packed.prove_device_stats(engine) == before
    _no_secrets_left(engine)


# ---------------------------------------------------------------- 7. the existing calls before and after
def test_the_existing_calls_before_and_after(bpp, engine):
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    t = 3
    params = _params(bpp, engine, t)
    d = _data(t, PATTERN * 2, 11)
    rows, _ = _rows(10)
    ps, cs = _plen(8, t), 32 * MS

    def existing():
        inp = _openings(packed, d, None, label=LABEL)
        proofs = torch.full((10, ps), 0xA5, dtype=torch.uint8, device="cuda")
        commits = torch.full((10, cs), 0xA5, dtype=torch.uint8, device="cuda")
        res = packed.prove_openings_device(params, inp, commitments_out=commits, proofs_out=proofs)
        assert res.rc == 0 and res.states is None
        host = _host(engine, params, packed, d, None, ps, cs, label=LABEL)
        # (bpp_prove_openings itself: the same call without the state rows)
        keep = {k: np.ascontiguousarray(d[k]) for k in ("values", "blind", "minv", "minp", "rng")}
        items = np.zeros(10, dtype=packed._PROVE_ITEM)
        items["values"], items["blindings32"], items["m"] = packed._rows(keep["values"]), packed._rows(keep["blind"]), d["m"]
        items["min_values"], items["min_present"] = packed._rows(keep["minv"]), packed._rows(keep["minp"])
        lbl = np.frombuffer(LABEL, dtype=np.uint8).copy()
        items["transcript_label"], items["label_len"] = lbl.ctypes.data, len(LABEL)
        items["rng_bytes"], items["rng_len"] = packed._rows(keep["rng"]), keep["rng"].shape[1]
        hp, hc = np.full((10, ps), 0xA5, dtype=np.uint8), np.full((10, cs), 0xA5, dtype=np.uint8)
        lens, codes, err = np.zeros(10, dtype=np.uintp), np.zeros(10, dtype=np.intc), ctypes.create_string_buffer(256)
        rc = engine.lib.bpp_prove_openings(engine.ctx, params.handle, items.ctypes.data_as(ctypes.POINTER(packed._lib.ProveItem)), 10, hc.ctypes.data, cs,
                                           hp.ctypes.data, ps, lens.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t)),
                                           codes.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), err, 256)
        assert rc == 0 and np.array_equal(hp, host["proofs"]) and np.array_equal(hc, host["commits"])
        return res.proofs.cpu().numpy(), res.commitments.cpu().numpy(), hp, hc

    first = existing()
    assert np.array_equal(first[0], first[2]) and np.array_equal(first[1], first[3])
    res = _device(params, packed, d, rows, ps, cs)
    assert res.rc == 0 and not np.array_equal(res.proofs.cpu().numpy(), first[0])  # (other transcripts: other proofs)
    d_bad = _data(t, PATTERN * 2, 11)
    bad = rows.copy()
    _bad_row(bad, 9, RATE)
    assert _device(params, packed, d_bad, bad, ps, cs).rc == INVALID_ARGUMENT
    again = existing()
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
