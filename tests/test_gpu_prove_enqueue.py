"""GPU tests of stream-ordered proving from device arrays on a resident plan (bpp_prove_plan_create / bpp_prove_enqueue).

THE CONTRACT: for every live item an enqueue writes what bpp_prove_openings_device_transcripts writes on the same arrays -- proof
bytes, commitment bytes, the status record, the state row, zeroed slots for failed and refused items -- and the summary record carries
that call's return code and message.  The reference of every byte comparison is that blocking call on the same engine and arrays;
every output buffer is prefilled with 0xA5 in both forms and compared whole, so every comparison is also the statement that no slack
byte was written.  N = 64, M_MAX = 8 throughout, except for the one finding no 64-bit value can produce ("Value exceeds bit vector
capacity!": those cases run at 32 bits, as the blocking form's own tests do)."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from oracle.pyref import merlin as M
from tests.helpers import LABEL

pytestmark = pytest.mark.gpu

N, M_MAX, MS = 64, 8, 8
INVALID_ARGUMENT, BAD_HANDLE = 2, -3
PATTERN = [1, 4, 2, 8, 1]
POSITIONS = [0, 1, 83, 164, 165]
RATE = 166
EMPTY, WRITTEN = 17, 1
L_ORDER = 2 ** 252 + 27742317777372353535851937790883648493
_CACHE = {}


@pytest.fixture(scope="module")
def packed():
    return importlib.import_module("bulletproofs-plus_amd.packed")


def _params(bpp, engine, t, n_bits=N):
    key = (id(engine), t, n_bits)
    if key not in _CACHE:
        _CACHE[key] = bpp.RangeParameters.init(n_bits, M_MAX, bpp.create_pedersen_gens_with_extension_degree(t), engine=engine)
    return _CACHE[key]


def _rounds(m, n_bits=N):
    return (n_bits * m).bit_length() - 1


def _plen(m, t, n_bits=N):
    return 1 + 32 * (t + 5 + 2 * _rounds(m, n_bits))


def _transcript(i, pos):
    """item i's transcript: a label of its own, one message whose length puts the sponge at `pos`"""
    def make(length):
        tr = M.Transcript(b"session %d" % i)
        tr.append_message(b"ctx", bytes([i & 255]) * length)
        return tr
    tr = make((pos - make(0).strobe.pos) % RATE)
    assert tr.strobe.pos == pos
    return tr


def _rows(n):
    """uint8 [n, 203]: all distinct, pos (byte 200) taking 0, 1, 83, 164 and 165 in turn"""
    if ("rows", n) not in _CACHE:
        rows = np.stack([np.frombuffer(_transcript(i, POSITIONS[i % 5]).strobe.to_bytes(), dtype=np.uint8) for i in range(n)])
        assert [int(r[200]) for r in rows] == [POSITIONS[i % 5] for i in range(n)] and len({bytes(r) for r in rows}) == n
        _CACHE[("rows", n)] = rows
    return _CACHE[("rows", n)].copy()


def _scalars(rng, shape):
    a = rng.integers(0, 256, size=tuple(shape) + (32,), dtype=np.uint8)
    a[..., 31] &= 0x0F  # < 2^252 < l
    return a


def _data(t, ms, seed, n_bits=N):
    """the arrays of a call, rows of MS entries; slack holds what would be a finding if it were read"""
    rng = np.random.default_rng(seed)
    n = len(ms)
    d = dict(t=t, n=n, n_bits=n_bits, m=np.array(ms, dtype=np.uint32))
    d["values"] = np.full((n, MS), 2 ** 64 - 1, dtype=np.uint64)
    d["blind"] = np.full((n, MS, t, 32), 0xFF, dtype=np.uint8)
    d["minv"] = np.full((n, MS), 2 ** 64 - 1, dtype=np.uint64)
    d["minp"] = np.full((n, MS), 0xFF, dtype=np.uint8)
    d["seeds"] = np.full((n, 32), 0xFF, dtype=np.uint8)
    d["seedp"] = np.zeros(n, dtype=np.uint8)
    d["rng"] = np.full((n, 32 * (_rounds(M_MAX, n_bits) + 3) + 8), 0xFF, dtype=np.uint8)
    for i, m in enumerate(ms):
        if m not in (1, 2, 4, 8):
            continue
        d["values"][i, :m] = rng.integers(0, 2 ** (n_bits - 1), size=m, dtype=np.uint64)
        d["blind"][i, :m] = _scalars(rng, (m, t))
        d["minp"][i, :m] = [(i + j) % 2 == 0 for j in range(m)]
        d["minv"][i, :m] = d["values"][i, :m] // 3
        if m == 1:
            d["seeds"][i] = _scalars(rng, ())
            d["seedp"][i] = 1
        need = 32 * (_rounds(m, n_bits) + 3)
        d["rng"][i, :need] = rng.integers(0, 256, size=need, dtype=np.uint8)
    return d


def _dev(a):
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _openings(packed, d, rows=None, commit=None, label=LABEL, cut=None):
    """cut: the arrays end behind row cut - 1 -- the tensors hold no more -- while the shapes say n rows"""
    keep = []

    def arr(a):
        if cut is None:
            return _dev(a)
        ten = _dev(a[:cut])
        keep.append(ten)
        return (ten.data_ptr(), a.shape)

    inp = packed.DeviceOpenings(arr(d["values"]), arr(d["blind"]), d["m"], commitments=None if commit is None else arr(commit),
                                min_values=arr(d["minv"]), min_present=arr(d["minp"]), seed_nonces=arr(d["seeds"]), seed_present=arr(d["seedp"]),
                                rng_bytes=arr(d["rng"]), label=label, item_states=None if rows is None else arr(rows))
    inp._cut_keep = keep
    return inp


def _plan(packed, engine, params, d, ps, cs, rows=False, commit=False, label=LABEL):
    return packed.ProvePlan(engine, params, d["m"], m_stride=MS, rng_stride=d["rng"].shape[1], commitments=commit, min_values=True,
                            min_present=True, seed_nonces=True, seed_present=True, label=label, item_states=rows, commit_stride=cs,
                            proof_stride=ps)


def _fresh(n, ps, cs):
    f = lambda *shape, dtype=torch.uint8: torch.full(shape, 0xA5 if dtype == torch.uint8 else -1515870811, dtype=dtype, device="cuda")  # noqa: E731
    return dict(proofs=f(n, ps), commits=f(n, cs), states=f(n, 203), status=f(n, 2, dtype=torch.int32), ok=f(n), summary=f(8, dtype=torch.int32))


def _blocking(packed, params, inp, n, ps, cs):
    o = _fresh(n, ps, cs)
    torch.cuda.synchronize()
    return packed.prove_openings_device(params, inp, commitments_out=o["commits"], proofs_out=o["proofs"], status_out=o["status"], states=o["states"])


def _enqueue(plan, inp, n, ps, cs, live=None, states=True, **kw):
    o = _fresh(n, ps, cs)
    torch.cuda.synchronize()
    return plan.enqueue(inp, live=live, states=o["states"] if states else False, commitments_out=o["commits"], proofs_out=o["proofs"],
                        status_out=o["status"], ok_mask=o["ok"], summary=o["summary"], **kw)


def _same(out, ref, plan, states=True):
    """everything the contract names against the blocking call's, whole buffers"""
    res = out.result()  # (waits for the ticket)
    n = plan.n
    got = {k: getattr(out, k).cpu().numpy() for k in ("proofs", "commitments", "status", "ok_mask")}
    want = {k: getattr(ref, k).cpu().numpy() for k in ("proofs", "commitments", "status")}
    assert list(plan.proof_lens) == list(ref.proof_lens)
    for k in ("proofs", "commitments", "status"):
        bad = [i for i in range(n) if not np.array_equal(got[k][i], want[k][i])]
        assert not bad, "%s: rows %s differ from bpp_prove_openings_device_transcripts on the same arrays" % (k, bad[:8])
    if states:
        gs, ws = out.states.cpu().numpy(), ref.states.cpu().numpy()
        bad = [i for i in range(n) if not np.array_equal(gs[i], ws[i])]
        assert not bad, "state rows %s differ from the blocking call's" % bad[:8]
    ok = (want["status"][:, 1] == 0)
    assert list(got["ok_mask"]) == [int(x) for x in ok], "ok_mask is not exactly the status-OK items"
    failing = [i for i in range(n) if want["status"][i, 1] != 0]
    assert res["flags"] == WRITTEN and res["code"] == ref.rc and res["msg"] == ref.message, (res, ref.rc, ref.message)
    assert res["index"] == (failing[0] if failing else 0)
    assert (res["n_ok"], res["n_failed"], res["n_empty"]) == (int(ok.sum()), len(failing), 0)
    if failing:
        assert res["msg_id"] == int(want["status"][failing[0], 1]) and ref.codes[failing[0]] == ref.rc
    return res


def _no_secrets_left(engine):
    examined, nonzero = ctypes.c_uint64(), ctypes.c_uint64()
    assert engine.lib.bpp_prove_secret_bytes(engine.ctx, ctypes.byref(examined), ctypes.byref(nonzero)) == 0
    assert examined.value > 0 and nonzero.value == 0


MS67 = (PATTERN * 14)[:67]


# ---------------------------------------------------------------- 1. parity, one transcript for the call
@pytest.mark.parametrize("t", [1, 3])
def test_parity_under_a_label_commitments_made_and_brought(bpp, engine, packed, t):
    params = _params(bpp, engine, t)
    d = _data(t, MS67, 100 + t)
    ps, cs = _plen(8, t) + 7, 32 * MS
    ref = _blocking(packed, params, _openings(packed, d), 67, ps, cs)
    assert ref.rc == 0, ref.message
    plan = _plan(packed, engine, params, d, ps, cs)
    try:
        assert not plan.host_status.any()
        out = _enqueue(plan, _openings(packed, d), 67, ps, cs)
        _same(out, ref, plan)
        assert len({bytes(r) for r in out.states.cpu().numpy()}) == 67
    finally:
        plan.close()
    # the same call bringing the commitments it made: the same bytes
    commit = np.full((67, MS, 32), 0xFF, dtype=np.uint8)
    made = ref.commitments.cpu().numpy().reshape(67, MS, 32)
    for i, m in enumerate(MS67):
        commit[i, :m] = made[i, :m]
    ref_b = _blocking(packed, params, _openings(packed, d, commit=commit), 67, ps, cs)
    assert ref_b.rc == 0 and np.array_equal(ref_b.proofs.cpu().numpy(), ref.proofs.cpu().numpy())
    plan = _plan(packed, engine, params, d, ps, cs, commit=True)
    try:
        _same(_enqueue(plan, _openings(packed, d, commit=commit), 67, ps, cs, shape_vector=True), ref_b, plan)
    finally:
        plan.close()
    _no_secrets_left(engine)


# ---------------------------------------------------------------- 2. parity, one transcript per item, states out
@pytest.mark.parametrize("t", [1, 3])
def test_parity_with_per_item_transcripts(bpp, engine, packed, t):
    params = _params(bpp, engine, t)
    d = _data(t, MS67, 110 + t)
    rows = _rows(67)
    ps, cs = _plen(8, t), 32 * MS + 1
    ref = _blocking(packed, params, _openings(packed, d, rows), 67, ps, cs)
    assert ref.rc == 0, ref.message
    plan = _plan(packed, engine, params, d, ps, cs, rows=True)
    try:
        _same(_enqueue(plan, _openings(packed, d, rows), 67, ps, cs), ref, plan)
        # without states_out: the same proofs, and nothing else is asked for
        out = _enqueue(plan, _openings(packed, d, rows), 67, ps, cs, states=False)
        _same(out, ref, plan, states=False)
        assert out.states is None
    finally:
        plan.close()
    _no_secrets_left(engine)


# ---------------------------------------------------------------- 3. a plan of one item
@pytest.mark.parametrize("rows_in", [False, True])
def test_one_item_plan(bpp, engine, packed, rows_in):
    t = 1
    params = _params(bpp, engine, t)
    d = _data(t, [1], 120)
    rows = _rows(1) if rows_in else None
    ps, cs = _plen(1, t) + 3, 32 * MS
    ref = _blocking(packed, params, _openings(packed, d, rows), 1, ps, cs)
    assert ref.rc == 0, ref.message
    plan = _plan(packed, engine, params, d, ps, cs, rows=rows_in)
    try:
        _same(_enqueue(plan, _openings(packed, d, rows), 1, ps, cs), ref, plan)
    finally:
        plan.close()
    _no_secrets_left(engine)


# ---------------------------------------------------------------- 4. findings
AT = (0, 63, 64, 66)  # the first item, the last, and either side of the sub-batch cut


def _spoil(d, rows, i, kind, n_bits):
    m = int(d["m"][i])
    if kind == "value":
        d["values"][i, m - 1] = 2 ** n_bits
    elif kind == "minimum":
        d["minp"][i, 0] = 1
        d["minv"][i, 0] = d["values"][i, 0] + np.uint64(1)
    elif kind == "blinding":
        d["blind"][i, m - 1, d["t"] - 1] = np.frombuffer(L_ORDER.to_bytes(32, "little"), dtype=np.uint8)
    elif kind == "nonce_aggregated":
        assert m == 2
        d["seeds"][i] = 0
        d["seedp"][i] = 1
    elif kind == "pos":
        rows[i] = 0xFF  # (nothing of the row but byte 200 may matter)
        rows[i, 200] = RATE


@pytest.mark.parametrize("kind,text,n_bits", [("value", "Value exceeds bit vector capacity!", 32), ("minimum", "Minimum value is larger than value", 64),
                                              ("blinding", "blinding factor is not canonical", 64),
                                              ("nonce_aggregated", "Mask recovery is not supported with an aggregated statement", 64),
                                              ("pos", "transcript state has pos >= rate", 64)])
def test_findings_at_the_ends_and_at_the_cut(bpp, engine, packed, kind, text, n_bits):
    t = 1
    params = _params(bpp, engine, t, n_bits)
    ms = list(MS67)
    if kind == "nonce_aggregated":
        for i in AT:
            ms[i] = 2
    d = _data(t, ms, 130, n_bits)
    rows = _rows(67)
    for i in AT:
        _spoil(d, rows, i, kind, n_bits)
    ps, cs = _plen(8, t, n_bits) + 3, 32 * MS
    ref = _blocking(packed, params, _openings(packed, d, rows), 67, ps, cs)
    assert [i for i in range(67) if ref.codes[i]] == list(AT) and ref.message == text
    plan = _plan(packed, engine, params, d, ps, cs, rows=True)
    try:
        out = _enqueue(plan, _openings(packed, d, rows), 67, ps, cs)
        res = _same(out, ref, plan)
        assert res["index"] == 0 and res["n_failed"] == 4 and res["msg"] == text
        got_p, got_c, got_s = out.proofs.cpu().numpy(), out.commitments.cpu().numpy(), out.states.cpu().numpy()
        for i in AT:
            used = int(plan.proof_lens[i])
            assert not got_p[i, :used].any() and (got_p[i, used:] == 0xA5).all()
            assert not got_c[i, :32 * ms[i]].any() and (got_c[i, 32 * ms[i]:] == 0xA5).all() and not got_s[i].any()
    finally:
        plan.close()
    _no_secrets_left(engine)


def test_an_m_no_statement_can_have_and_a_later_finding(bpp, engine, packed):
    t = 1
    params = _params(bpp, engine, t)
    ms = [1, 4, 3, 8, 1, 2, 16, 1]
    d = _data(t, ms, 140)
    rows = _rows(8)
    rows[2] = 0xFF  # (a refused item's row is never read)
    _spoil(d, rows, 5, "blinding", 64)
    ps, cs = _plen(8, t), 32 * MS
    ref = _blocking(packed, params, _openings(packed, d, rows), 8, ps, cs)
    assert [int(c != 0) for c in ref.codes] == [0, 0, 1, 0, 0, 1, 1, 0] and ref.message == "Number of commitments must be a power of two"
    plan = _plan(packed, engine, params, d, ps, cs, rows=True)
    try:
        assert [int(c != 0) for c in plan.host_status] == [0, 0, 1, 0, 0, 0, 1, 0]
        res = _same(_enqueue(plan, _openings(packed, d, rows), 8, ps, cs), ref, plan)
        assert res["index"] == 2 and res["n_failed"] == 3 and res["n_ok"] == 5
    finally:
        plan.close()


def test_every_item_fails(bpp, engine, packed):
    t = 1
    params = _params(bpp, engine, t)
    d = _data(t, PATTERN, 150)
    rows = _rows(5)
    for i in range(5):
        _spoil(d, rows, i, "blinding", 64)
    ps, cs = _plen(8, t), 32 * MS
    ref = _blocking(packed, params, _openings(packed, d, rows), 5, ps, cs)
    assert all(ref.codes)
    plan = _plan(packed, engine, params, d, ps, cs, rows=True)
    try:
        out = _enqueue(plan, _openings(packed, d, rows), 5, ps, cs)
        res = _same(out, ref, plan)
        assert res["n_failed"] == 5 and res["n_ok"] == 0 and res["index"] == 0 and not out.ok_mask.cpu().numpy().any()
    finally:
        plan.close()
    _no_secrets_left(engine)


# ---------------------------------------------------------------- 5. the live mask
def _loud(d, rows, dead):
    """copies in which every dead row holds 0xFF: a value and a promise no item may have, scalars that are not canonical, a nonce flag
    on aggregated items, a state at pos 255 -- each a finding if it were read"""
    e = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    r = rows.copy()
    for i in dead:
        for k in ("values", "blind", "minv", "minp", "seeds", "seedp", "rng"):
            e[k][i] = e[k].dtype.type(2 ** 64 - 1) if e[k].dtype == np.uint64 else 0xFF
        r[i] = 0xFF
    return e, r


@pytest.mark.parametrize("t", [1, 3])
def test_live_mask_dead_rows_are_never_read(bpp, engine, packed, t):
    params = _params(bpp, engine, t)
    d = _data(t, MS67, 160 + t)
    rows = _rows(67)
    ps, cs = _plen(8, t) + 5, 32 * MS
    ref = _blocking(packed, params, _openings(packed, d, rows), 67, ps, cs)  # (dead rows hold valid data here)
    assert ref.rc == 0, ref.message
    mask = np.array([0 if (i % 3 == 1 or i >= 60) else (1 + i % 255) for i in range(67)], dtype=np.uint8)
    dead = [i for i in range(67) if not mask[i]]
    last_live = max(i for i in range(67) if mask[i])
    assert last_live == 59 and 0 not in dead
    loud, loud_rows = _loud(d, rows, dead)
    plan = _plan(packed, engine, params, d, ps, cs, rows=True)
    try:
        out = _enqueue(plan, _openings(packed, loud, loud_rows, cut=last_live + 1), 67, ps, cs, live=_dev(mask))
        res = out.result()
        assert (res["code"], res["msg_id"], res["index"], res["flags"]) == (0, 0, 0, WRITTEN)
        assert (res["n_ok"], res["n_failed"], res["n_empty"]) == (67 - len(dead), 0, len(dead))
        got = {k: getattr(out, k).cpu().numpy() for k in ("proofs", "commitments", "status", "ok_mask", "states")}
        want = {k: getattr(ref, k).cpu().numpy() for k in ("proofs", "commitments", "status", "states")}
        for i in range(67):
            used, m = int(plan.proof_lens[i]), MS67[i]
            if mask[i]:
                for k in want:
                    assert np.array_equal(got[k][i], want[k][i]), "live item %d: %s differs from the blocking call's" % (i, k)
            else:
                assert not got["proofs"][i, :used].any() and (got["proofs"][i, used:] == 0xA5).all()
                assert not got["commitments"][i, :32 * m].any() and (got["commitments"][i, 32 * m:] == 0xA5).all()
                assert not got["states"][i].any() and list(got["status"][i]) == [0, EMPTY]
        assert list(got["ok_mask"]) == [int(x != 0) for x in mask]
        # all dead: nothing but the mask is read -- every array holds one row, 0xFF throughout
        none = np.zeros(67, dtype=np.uint8)
        every, every_rows = _loud(d, rows, range(67))
        out = _enqueue(plan, _openings(packed, every, every_rows, cut=1), 67, ps, cs, live=_dev(none))
        res = out.result()
        assert (res["code"], res["n_ok"], res["n_failed"], res["n_empty"]) == (0, 0, 0, 67)
        st = out.status.cpu().numpy()
        assert (st[:, 0] == 0).all() and (st[:, 1] == EMPTY).all() and not out.ok_mask.cpu().numpy().any() and not out.states.cpu().numpy().any()
        r = packed._lib.ShardResult()
        rec = np.ascontiguousarray(st[0:1])
        assert engine.lib.bpp_prove_status_result(rec.ctypes.data_as(ctypes.POINTER(packed._lib.DeviceProveStatus)), ctypes.byref(r)) == 0
        assert r.code == 0 and r.tier == 0
    finally:
        plan.close()
    _no_secrets_left(engine)


# ---------------------------------------------------------------- 6. steady state
def test_steady_state_allocates_nothing_and_waits_for_nothing(bpp, engine, packed):
    t = 1
    params = _params(bpp, engine, t)
    ps, cs = _plen(8, t), 32 * MS
    ds = [_data(t, MS67, 170 + k) for k in range(3)]
    rows = [np.roll(_rows(67), k, axis=0) for k in range(3)]
    # call 2 fails items that call 3 proves: nothing of it may be left in call 3's outputs
    _spoil(ds[1], rows[1], 7, "blinding", 64)
    _spoil(ds[1], rows[1], 64, "pos", 64)
    ref = _blocking(packed, params, _openings(packed, ds[2], rows[2]), 67, ps, cs)
    assert ref.rc == 0
    plan = _plan(packed, engine, params, ds[0], ps, cs, rows=True)
    try:
        inps = [_openings(packed, ds[k], rows[k]) for k in range(3)]
        o = _fresh(67, ps, cs)
        torch.cuda.synchronize()
        kw = dict(states=o["states"], commitments_out=o["commits"], proofs_out=o["proofs"], status_out=o["status"], ok_mask=o["ok"],
                  summary=o["summary"])
        first = plan.enqueue(inps[0], **kw)
        s1 = packed.prove_enqueue_stats(engine)
        second = plan.enqueue(inps[1], **kw)  # (the same output buffers: stream order alone keeps the calls apart)
        third = plan.enqueue(inps[2], **kw)
        s3 = packed.prove_enqueue_stats(engine)  # (before any wait)
        assert s3["host_waits"] == 0 and s3["calls"] == s1["calls"] + 2
        assert s3["allocations"] == s1["allocations"] and s3["first_calls"] == s1["first_calls"]
        assert second.ticket == first.ticket + 1 and third.ticket == second.ticket + 1
        _same(third, ref, plan)
        assert first.done() and second.done()
        _no_secrets_left(engine)
    finally:
        plan.close()


# ---------------------------------------------------------------- 7. the loop on one stream
def test_prove_refill_verify_on_one_stream(bpp, packed):
    t = 1
    n = 67
    ps, cs = _plen(8, t), 32 * MS
    d0, d1 = _data(t, MS67, 180), _data(t, MS67, 181)
    rows0, rows1 = _rows(n), np.roll(_rows(n), 3, axis=0)
    _spoil(d1, rows1, 20, "blinding", 64)  # one item fails ...
    mask = np.ones(n, dtype=np.uint8)
    mask[[5, 40]] = 0                      # ... and two are switched off
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        eng = bpp.Engine(0, stream=stream.cuda_stream)
        params = bpp.RangeParameters.init(N, M_MAX, bpp.create_pedersen_gens_with_extension_degree(t), engine=eng)
        try:
            # the blocking prover on both sets: the resident batch's first contents, and the reference of the step
            ref0 = _blocking(packed, params, _openings(packed, d0, rows0), n, ps, cs)
            ref1 = _blocking(packed, params, _openings(packed, d1, rows1), n, ps, cs)
            assert ref0.rc == 0 and [i for i in range(n) if ref1.codes[i]] == [20]
            live = [i for i in range(n) if mask[i] and i != 20]
            sel = torch.tensor(live, device="cuda")
            fresh = packed.DeviceMixedInput(ref1.proofs[sel].contiguous(), ref1.proof_lens[live], d1["m"][live],
                                            ref1.commitments.view(n, MS, 32)[sel].contiguous(), min_values=_dev(d1["minv"][live]),
                                            min_present=_dev(d1["minp"][live]), seed_nonces=_dev(d1["seeds"][live]),
                                            seed_present=_dev(d1["seedp"][live]), item_states=_dev(rows1[live]))
            packed.verify_batch_mixed_device(params, fresh)  # (raises unless every proof verifies under its own transcript)
            chunk = 16
            bounds = list(range(0, n, chunk)) + [n]
            cut = [sum(1 for i in live if i < b) for b in bounds]  # the same groups over the live items alone
            assert all(cut[g + 1] > cut[g] for g in range(len(cut) - 1))
            rb_ref = packed.ResidentBatch.from_mixed(params, fresh)
            want = rb_ref.enqueue(bounds=cut, states=True)
            want_records, want_states = want.results(), want.states.cpu().numpy()
            rb_ref.close()
            assert all(r["code"] == 0 for r in want_records)

            rb = packed.ResidentBatch.from_mixed(params, ref0.as_mixed_input())
            rb.enqueue(bounds=bounds, states=True).wait()  # (the layout is planned here, with nothing in flight)
            plan = _plan(packed, eng, params, d0, ps, cs, rows=True)
            src = _openings(packed, d1, rows1)           # what a producer made ...
            dst = _openings(packed, d0, rows0)           # ... and the buffers the plan's step reads
            mask_dev, mask_src = torch.ones(n, dtype=torch.uint8, device="cuda"), _dev(mask)
            # a first step with every item live: the plan's first call, the batch's first refill under a mask, its layout
            warm = plan.enqueue(dst, live=mask_dev, states=True)
            rb.refill(warm.as_mixed_input(), shape_vectors=False)
            warmed = rb.enqueue(bounds=bounds, states=True)
            assert all(r["code"] == 0 for r in warmed.results()) and warm.result()["n_ok"] == n
            torch.cuda.synchronize()
            p0, r0, e0 = packed.prove_enqueue_stats(eng), packed.refill_stats(eng), packed.enqueue_stats(eng)
            # ---- the step: a device-side copy fills the openings, prove, refill under the prover's ok mask, verify; no wait between
            for a, b in zip(dst._keep, src._keep):
                a.copy_(b)
            mask_dev.copy_(mask_src)
            proved = plan.enqueue(dst, live=mask_dev, states=True)
            filled = rb.refill(proved.as_mixed_input(), shape_vectors=False)
            checked = rb.enqueue(bounds=bounds, states=True)
            p1, r1, e1 = packed.prove_enqueue_stats(eng), packed.refill_stats(eng), packed.enqueue_stats(eng)
            checked.wait()  # the one wait of the step
            assert p1["host_waits"] == p0["host_waits"] == 0 and p1["calls"] == p0["calls"] + 1 and p1["allocations"] == p0["allocations"]
            assert r1["host_waits"] == r0["host_waits"] and e1["host_waits"] == e0["host_waits"] == 0
            assert proved.done() and filled.done()
            assert filled.result()["code"] == 0
            got_records, got_states = checked.results(), checked.states.cpu().numpy()
            assert [r["code"] for r in got_records] == [0] * (len(bounds) - 1), got_records
            assert [(r["code"], r["tier"]) for r in got_records] == [(r["code"], r["tier"]) for r in want_records]
            assert np.array_equal(got_states[live], want_states)
            off = [i for i in range(n) if i not in live]
            assert not got_states[off].any()
            assert list(proved.ok_mask.cpu().numpy()) == [int(i in live) for i in range(n)]
            res = proved.result()
            assert res["index"] == 20 and res["msg"] == "blinding factor is not canonical" and (res["n_ok"], res["n_failed"], res["n_empty"]) == (n - 3, 1, 2)
            # the prover's outputs for the live items are the blocking prover's
            got_p, want_p = proved.proofs.cpu().numpy(), ref1.proofs.cpu().numpy()
            assert all(np.array_equal(got_p[i, :int(plan.proof_lens[i])], want_p[i, :int(plan.proof_lens[i])]) for i in live)
            plan.close()
            rb.close()
        finally:
            params.close()
            eng.close()


# ---------------------------------------------------------------- 8. refusals
def test_refusals_before_any_launch(bpp, engine, packed, opt):
    t = 1
    params = _params(bpp, engine, t)
    d = _data(t, PATTERN, 190)
    rows = _rows(5)
    ps, cs = _plen(8, t), 32 * MS
    plan = _plan(packed, engine, params, d, ps, cs, rows=True)
    plain = _plan(packed, engine, params, d, ps, cs, rows=False)
    lib = engine.lib
    try:
        assert _enqueue(plan, _openings(packed, d, rows), 5, ps, cs).result()["code"] == 0
        before = packed.prove_enqueue_stats(engine)
        o = _fresh(5, ps, cs)
        dev_rows = _dev(rows)
        host = np.zeros(5 * max(ps, 203), dtype=np.uint8)
        torch.cuda.synchronize()
        alive = []

        def call(handle=None, inp=None, st=None, **kw):
            inp = _openings(packed, d, rows) if inp is None else inp
            st = inp.struct_without_transcript() if st is None else st
            if "m" not in kw:
                st.m = None
            a = dict(item_states=dev_rows.data_ptr(), live=None, commits=o["commits"].data_ptr(), proofs=o["proofs"].data_ptr(),
                     states=o["states"].data_ptr(), status=o["status"].data_ptr(), ok=o["ok"].data_ptr(), summary=o["summary"].data_ptr())
            a.update({k: v for k, v in kw.items() if k != "m"})
            p = lambda v: None if v is None else ctypes.c_void_p(int(v))  # noqa: E731
            ticket = ctypes.c_uint64()
            rc = lib.bpp_prove_enqueue(engine.ctx, plan.handle if handle is None else handle, ctypes.byref(st), p(a["item_states"]), p(a["live"]),
                                       p(a["commits"]), p(a["proofs"]), p(a["states"]), p(a["status"]), p(a["ok"]), p(a["summary"]),
                                       ctypes.byref(ticket))
            alive.append(inp)  # (an accepted call reads the arrays after it has returned)
            return rc, (lib.bpp_ctx_last_error(engine.ctx) or b"").decode()

        def refused(needle, **kw):
            rc, msg = call(**kw)
            assert rc == INVALID_ARGUMENT and needle in msg, (needle, rc, msg)

        assert call()[0] == 0
        before["calls"] += 1
        # memory that is not this device's, field by field
        for field in ("item_states", "live", "commits", "proofs", "states", "status", "ok", "summary"):
            name = {"item_states": "item_states_dev", "live": "live_dev", "commits": "commitments_out_dev", "proofs": "proofs_out_dev",
                    "states": "states_out_dev", "status": "status_dev", "ok": "ok_mask_dev", "summary": "summary_dev"}[field]
            refused(name + " is not device memory", **{field: host.ctypes.data})
        host_values = np.ascontiguousarray(d["values"])
        st = _openings(packed, d, rows).struct_without_transcript()
        st.values = host_values.ctypes.data
        refused("values is not device memory", st=st)
        refused("proofs_out_dev is null", proofs=None)
        refused("commitments_out_dev is null", commits=None)
        # item_states_dev against the flag, both ways
        refused("item_states_dev is null", item_states=None)
        rc, msg = call(handle=plain.handle)
        assert rc == INVALID_ARGUMENT and "item_states_dev is given" in msg
        # an optional array given or absent against the plan
        st = _openings(packed, d, rows).struct_without_transcript()
        st.seed_present = None
        refused("seed_present is null", st=st)
        commit = np.zeros((5, MS, 32), dtype=np.uint8)
        refused("commitments32 is given", inp=_openings(packed, d, rows, commit=commit))
        # a shape field that differs
        for field, value in (("n_items", 4), ("m_stride", MS - 1), ("rng_stride", d["rng"].shape[1] - 1)):
            st = _openings(packed, d, rows).struct_without_transcript()
            setattr(st, field, value)
            refused(field + " differs", st=st)
        other = d["m"].copy()
        other[3] = 4
        st = _openings(packed, d, rows).struct_without_transcript()
        st.m = other.ctypes.data
        refused("m[3] differs", st=st, m=True)
        st = _openings(packed, d, rows).struct_without_transcript()
        keep_m = d["m"].copy()
        st.m = keep_m.ctypes.data
        assert call(st=st, m=True)[0] == 0  # (an equal host array passes)
        before["calls"] += 1
        # overlapping state ranges
        both = torch.zeros(2 * 5 * 203, dtype=torch.uint8, device="cuda")
        both[:5 * 203] = dev_rows.reshape(-1)
        torch.cuda.synchronize()
        refused("overlap", item_states=both.data_ptr(), states=both.data_ptr() + 4 * 203)
        refused("overlap", item_states=both.data_ptr(), states=both.data_ptr())
        assert call(item_states=both.data_ptr(), states=both.data_ptr() + 5 * 203)[0] == 0  # (end to end is no overlap)
        before["calls"] += 1
        # an unknown plan
        rc, _ = call(handle=plan.handle + 1000)
        assert rc == BAD_HANDLE
        assert lib.bpp_prove_plan_destroy(engine.ctx, plan.handle + 1000) == BAD_HANDLE
        torch.cuda.synchronize()
        assert packed.prove_enqueue_stats(engine) == before
        # creation: prove_check = 1 with the blocking call's text, a bad whole-call state, transcript fields under the flag
        opt("prove_check", 1)
        with pytest.raises(bpp.ProofError, match="prove_check = 1 is not supported"):
            _plan(packed, engine, params, d, ps, cs)
        opt("prove_check", -1)
        bad_state = bytearray(_transcript(1, 1).strobe.to_bytes())
        bad_state[200] = RATE
        with pytest.raises(bpp.ProofError, match="transcript state has pos >= rate"):
            packed.ProvePlan(engine, params, d["m"], m_stride=MS, rng_stride=d["rng"].shape[1], state=bytes(bad_state), commit_stride=cs, proof_stride=ps)
        with pytest.raises(bpp.ProofError, match="m_stride is below"):
            packed.ProvePlan(engine, params, d["m"], m_stride=4, rng_stride=d["rng"].shape[1], commit_stride=cs, proof_stride=ps)
    finally:
        plan.close()
        plain.close()
    _no_secrets_left(engine)


# ---------------------------------------------------------------- 9. the blocking call and the plan: one shape step
def test_both_forms_one_shape(bpp, engine, packed):
    """m = [1, 4, 3, 2, 0, 8, 1, 4] under m_max = 4, a proof_stride that holds m = 2 and a commit_stride of 128: the m = 4 items are
    refused for the stride (their commitment slots are zeroed, their proof slots are not touched), 3, 0 and 8 have no proof length
    (nothing of theirs is touched).  Lengths, host findings, every output row and every status record: equal between the forms."""
    t, m_max = 1, 4
    key = (id(engine), "m_max", m_max, t)
    if key not in _CACHE:
        _CACHE[key] = bpp.RangeParameters.init(N, m_max, bpp.create_pedersen_gens_with_extension_degree(t), engine=engine)
    params = _CACHE[key]
    ms = [1, 4, 3, 2, 0, 8, 1, 4]
    refused, stride_refused, proved = [1, 2, 4, 5, 7], [1, 7], [0, 3, 6]
    d = _data(t, ms, 200)
    rows = _rows(8)
    ps, cs = _plen(2, t), 128
    lens = [_plen(1, t), _plen(4, t), 0, _plen(2, t), 0, 0, _plen(1, t), _plen(4, t)]
    ref = _blocking(packed, params, _openings(packed, d, rows), 8, ps, cs)
    assert list(ref.proof_lens) == lens
    assert [i for i in range(8) if ref.codes[i]] == refused and ref.message == "proof_stride too small"
    plan = _plan(packed, engine, params, d, ps, cs, rows=True)
    try:
        assert list(plan.proof_lens) == lens
        assert [int(c) for c in plan.host_status] == [int(c) for c in ref.codes]  # (every finding of this call is the host's)
        out = _enqueue(plan, _openings(packed, d, rows), 8, ps, cs)
        res = _same(out, ref, plan)
        assert (res["index"], res["n_ok"], res["n_failed"]) == (1, 3, 5)
        for form in (ref, out):
            p, c, s, st = (getattr(form, k).cpu().numpy() for k in ("proofs", "commitments", "states", "status"))
            assert [int(x) for x in st[:, 1]] == [0, 4, 1, 0, 1, 2, 0, 4]  # proof_stride, power of two, generators
            assert [int(x) for x in st[:, 0]] == [int(x) for x in ref.codes]
            for i in stride_refused:  # BPP_PROVE_ROW_ZERO_COMMIT alone
                assert (p[i] == 0xA5).all() and not c[i].any() and not s[i].any()
            for i in (2, 4, 5):       # no flag
                assert (p[i] == 0xA5).all() and (c[i] == 0xA5).all() and not s[i].any()
            for i in proved:
                assert (p[i, :lens[i]] != 0xA5).any() and (p[i, lens[i]:] == 0xA5).all()
                assert (c[i, :32 * ms[i]] != 0xA5).any() and (c[i, 32 * ms[i]:] == 0xA5).all() and s[i].any()
    finally:
        plan.close()
    _no_secrets_left(engine)


# ---------------------------------------------------------------- 10. two faults in one call: the earlier refusal wins
def test_refusal_precedence(bpp, engine, packed, opt):
    t = 1
    params = _params(bpp, engine, t)
    d = _data(t, PATTERN, 210)
    rows = _rows(5)
    ps, cs = _plen(8, t), 32 * MS
    lib = engine.lib
    plan = _plan(packed, engine, params, d, ps, cs, rows=True)
    try:
        inp = _openings(packed, d, rows)
        o = _fresh(5, ps, cs)
        dev_m = torch.from_numpy(d["m"].view(np.int32).copy()).cuda()
        both = torch.zeros(2 * 5 * 203, dtype=torch.uint8, device="cuda")
        host = np.zeros(5 * 203, dtype=np.uint8)
        bad_state = np.frombuffer(_transcript(1, 1).strobe.to_bytes(), dtype=np.uint8).copy()
        bad_state[200] = RATE
        label = np.frombuffer(LABEL, dtype=np.uint8).copy()
        torch.cuda.synchronize()
        stats = lambda: (packed.prove_device_stats(engine), packed.prove_enqueue_stats(engine))  # noqa: E731
        before = stats()
        p = lambda v: None if v is None else ctypes.c_void_p(int(v))  # noqa: E731
        TOO_MANY, UNKNOWN = 2 ** 24 + 1, int(getattr(params.handle, "value", params.handle)) + 1000

        def blocking(needle, rc_want=INVALID_ARGUMENT, handle=params.handle, item_states=inp.item_states, states=None, **fields):
            st = inp.struct_without_transcript()
            for k, v in fields.items():
                setattr(st, k, v)
            lens = np.zeros(5, dtype=np.uintp)
            err = ctypes.create_string_buffer(256)
            rc = lib.bpp_prove_openings_device_transcripts(engine.ctx, handle, ctypes.byref(st), item_states, o["commits"].data_ptr(), cs,
                                                           o["proofs"].data_ptr(), ps, lens.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t)),
                                                           p(states), None, None, err, 256)
            assert rc == rc_want and needle in err.value.decode(), (needle, rc, err.value.decode())

        def create(needle, rc_want=INVALID_ARGUMENT, handle=params.handle, flags=1, **fields):
            shape = packed._lib.ProveArrays(5, d["m"].ctypes.data, MS, 1, 1, None, 1, 1, 1, 1, 1, d["rng"].shape[1], None, None, 0)
            for k, v in fields.items():
                setattr(shape, k, v)
            made = ctypes.c_uint64()
            err = ctypes.create_string_buffer(256)
            rc = lib.bpp_prove_plan_create(engine.ctx, handle, ctypes.byref(shape), cs, ps, flags, ctypes.byref(made), err, 256)
            if rc == 0:
                lib.bpp_prove_plan_destroy(engine.ctx, made.value)
            assert rc == rc_want and needle in err.value.decode(), (needle, rc, err.value.decode())

        # ---- the blocking call, in its order
        blocking("values is not device memory", values=host.ctypes.data, m=None)
        blocking("null argument", m=None, m_stride=0)
        blocking("m must be host memory", m=dev_m.data_ptr(), m_stride=0)
        opt("prove_check", 1)
        blocking("m_stride is 0", m_stride=0)
        blocking("prove_check = 1 is not supported", transcript_label=label.ctypes.data, label_len=len(LABEL))
        create("m_stride is 0", m_stride=0)
        create("prove_check = 1 is not supported", transcript_label=label.ctypes.data, label_len=len(LABEL))
        opt("prove_check", -1)
        blocking("transcript_state / transcript_label must be null", transcript_state=bad_state.ctypes.data)
        blocking("transcript state has pos >= rate", item_states=None, transcript_state=bad_state.ctypes.data, handle=UNKNOWN)
        blocking("overlap", item_states=p(both.data_ptr()), states=both.data_ptr() + 4 * 203, handle=UNKNOWN)
        blocking("overlap", item_states=p(both.data_ptr()), states=both.data_ptr() + 4 * 203, n_items=TOO_MANY)
        blocking("unknown params handle", BAD_HANDLE, handle=UNKNOWN, n_items=TOO_MANY)
        blocking("batch too large", 5, n_items=TOO_MANY)  # (m holds five entries: the cap comes before m is read)
        blocking("m_stride is below", m_stride=4)
        # ---- bpp_prove_plan_create, in its order
        create("unknown flag", flags=3, m=None)
        create("null argument", m=None, m_stride=0)
        create("m must be host memory", m=dev_m.data_ptr(), m_stride=0)
        create("transcript_state / transcript_label must be null", transcript_state=bad_state.ctypes.data)
        create("transcript state has pos >= rate", flags=0, transcript_state=bad_state.ctypes.data, handle=UNKNOWN)
        create("unknown params handle", BAD_HANDLE, handle=UNKNOWN, n_items=TOO_MANY)
        create("batch too large", 5, n_items=TOO_MANY)
        create("m_stride is below", m_stride=4)
        # ---- bpp_prove_enqueue: a pointer kind before the plan's own refusals
        st = inp.struct_without_transcript()
        st.m, st.n_items = None, 4
        ticket = ctypes.c_uint64()
        rc = lib.bpp_prove_enqueue(engine.ctx, plan.handle, ctypes.byref(st), inp.item_states, None, p(o["commits"].data_ptr()),
                                   p(o["proofs"].data_ptr()), p(o["states"].data_ptr()), p(o["status"].data_ptr()), p(o["ok"].data_ptr()),
                                   p(host.ctypes.data), ctypes.byref(ticket))
        msg = (lib.bpp_ctx_last_error(engine.ctx) or b"").decode()
        assert rc == INVALID_ARGUMENT and "summary_dev is not device memory" in msg, (rc, msg)
        assert stats() == before  # nothing was counted: nothing was launched
        for buf in o.values():
            assert (buf.cpu().numpy().view(np.uint8) == 0xA5).all()
    finally:
        plan.close()


# ---------------------------------------------------------------- 11. one ticket ring behind every stream call
def test_seventy_tickets_from_three_issuers(bpp, packed):
    t, ps, cs = 1, _plen(1, 1), 32 * MS
    d, rows = _data(t, [1], 220), _rows(1)
    eng = bpp.Engine(0)
    params = bpp.RangeParameters.init(N, M_MAX, bpp.create_pedersen_gens_with_extension_degree(t), engine=eng)
    try:
        ref = _blocking(packed, params, _openings(packed, d, rows), 1, ps, cs)
        assert ref.rc == 0, ref.message
        rb = packed.ResidentBatch.from_mixed(params, ref.as_mixed_input())
        plan = _plan(packed, eng, params, d, ps, cs, rows=True)
        inp = _openings(packed, d, rows)
        row, word = _dev(rows), torch.zeros((1, 4), dtype=torch.uint8, device="cuda")
        first = rb.enqueue(bounds=[0, 1], states=True)  # (the context's first ticket; the weights bpp_enqueue_weights copies)
        tickets = [first.ticket]
        while len(tickets) < 70:
            k = len(tickets) % 3
            if k == 0:
                tickets.append(packed.transcript_ops(eng, row, [packed.TAppend(b"ctx", word)]).ticket)
            elif k == 1:
                tickets.append(plan.enqueue(inp, states=True).ticket)
            else:
                tickets.append(rb.enqueue_weights().ticket)
        assert tickets == list(range(tickets[0], tickets[0] + 70))
        done = ctypes.c_int(-1)
        lib = eng.lib
        assert lib.bpp_enqueue_wait(eng.ctx, tickets[-1]) == 0
        for tk in tickets[-64:]:
            assert lib.bpp_enqueue_done(eng.ctx, tk, ctypes.byref(done)) == 0 and done.value == 1
        for tk in (0, tickets[-1] + 1):
            assert lib.bpp_enqueue_done(eng.ctx, tk, ctypes.byref(done)) == BAD_HANDLE
            assert lib.bpp_enqueue_wait(eng.ctx, tk) == BAD_HANDLE
        assert packed.prove_enqueue_stats(eng)["allocations"] == 0  # (the verifier's enqueue made the events)
        plan.close()
        rb.close()
    finally:
        params.close()
        eng.close()
