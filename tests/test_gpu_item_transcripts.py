"""GPU tests: per-item transcripts on the device paths (include/bpp.h, csrc/item_states.h) -- in at upload and refill
(bpp_batch_upload_packed_device_transcripts, _mixed_device_transcripts, bpp_batch_refill_enqueue_transcripts, _mixed_transcripts),
out at enqueue (bpp_verify_enqueue_states).

References: for an upload, bpp_batch_upload on the equivalent ITEM array (item i under transcript_state = row i); for a refill, a
FRESH upload with transcripts of the rows in question (all of them, the first c, each group's live rows alone in slot order); for the
rows bpp_verify_enqueue_states hands out, bpp_verify_batch_states.  A batch is never compared with its own output.

The corpus: n_bits = 32, m_max = 4; 70 slots at t = 1 under the boundaries [0, 5, 33, 70] -- packed corpora of m = 1, mixed corpora in
the pattern [4, 1, 2, 1, 1, 4, 2] -- and 9 mixed slots at t = 2.  Every proof is made by the engine's prover under ITS OWN transcript:
Transcript::new(LABEL) plus one context message per item whose length differs from item to item, so the rows' `pos` differ; slot 41
sits at pos = 165, the last position of the block (the length is searched on the host).  Every verification runs under both PASS-1
kernels ("transcripts_wave" 0 and 1)."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from oracle.pyref import merlin as M
from oracle.pyref import protocol as O
from tests.helpers import LABEL, Prng, sb

pytestmark = pytest.mark.gpu

L_BYTES = np.frombuffer(bytes.fromhex("edd3f55c1a631258d69cf7a2def9de14" + "00" * 15 + "10"), dtype=np.uint8)  # the group order
PATTERN = [4, 1, 2, 1, 1, 4, 2]
M_STRIDE = 4
N, BOUNDS = 70, [0, 5, 33, 70]
N2 = 9
STROBE_R = 166
POS_SLOT = 41  # the slot whose row sits at pos = STROBE_R - 1
CTX_LABEL = b"tx"
D1, R1 = 1, 1 + 32 * 4  # t = 1: [t] d1 A A1 B r1 s1 (L R)*
WAVES = (0, 1)


@pytest.fixture(scope="module")
def packed():
    return importlib.import_module("bulletproofs-plus_amd.packed")


def _context(bpp, name, i, length):
    tr = bpp.Transcript.new(LABEL)
    unit = b"%s/%d/" % (name, i)
    tr.append_message(CTX_LABEL, (unit * (length // len(unit) + 1))[:length])
    return tr


def _length_for_pos(bpp, pos):
    for length in range(8, 8 + 2 * STROBE_R):
        if _context(bpp, b"search", 0, length).state[200] == pos:
            return length
    raise AssertionError("no context length gives pos %d" % pos)


def _prove(bpp, params, n_bits, t, ms, name):
    """rows of len(ms) items, each proved under its own transcript by ONE bpp_prove_batch_mixed call"""
    rng = Prng(b"item-transcripts-" + name)
    count = len(ms)
    last = _length_for_pos(bpp, STROBE_R - 1)
    trs, sts, ws, exts, blinds, opened = [], [], [], [], [], []
    commitments = np.zeros((count, M_STRIDE, 32), dtype=np.uint8)
    min_values = np.zeros((count, M_STRIDE), dtype=np.uint64)
    min_present = np.zeros((count, M_STRIDE), dtype=np.uint8)
    seeds = np.zeros((count, 32), dtype=np.uint8)
    for i, m in enumerate(ms):
        rounds = (n_bits * m).bit_length() - 1
        vals = [rng.next_u64() % (1 << min(n_bits, 63)) for _ in range(m)]
        bl = [[sb(O.random_not_zero(rng)) for _ in range(t)] for _ in range(m)]
        mins = [(v // 3 if (i + j) % 3 == 0 else None) for j, v in enumerate(vals)]
        nonce = sb(O.random_not_zero(rng)) if m == 1 else None
        comms = params.commit_many(vals, bl)
        trs.append(_context(bpp, name, i, last if i == POS_SLOT else 8 + (7 * i) % 61))
        sts.append(bpp.RangeStatement.init(params, comms, mins, nonce))
        ws.append(bpp.RangeWitness.init([bpp.CommitmentOpening.new(vals[j], bl[j]) for j in range(m)]))
        exts.append(rng.fill_bytes(32 * (rounds + 3)))
        blinds.append(b"".join(bl[0]))
        opened.append((vals, bl, mins, nonce))
        commitments[i, :m] = np.frombuffer(b"".join(comms), dtype=np.uint8).reshape(m, 32)
        for j, v in enumerate(mins):
            if v is not None:
                min_values[i, j], min_present[i, j] = v, 1
        if nonce is not None:
            seeds[i] = np.frombuffer(nonce, dtype=np.uint8)
    raw = [g.to_bytes() for g in bpp.RangeProof.prove_batch_mixed(trs, sts, ws, exts)]
    lens = np.array([len(r) for r in raw], dtype=np.uintp)
    proofs = np.zeros((count, int(lens.max())), dtype=np.uint8)
    for i, r in enumerate(raw):
        proofs[i, :len(r)] = np.frombuffer(r, dtype=np.uint8)
    blind_rows = np.zeros((count, t, 32), dtype=np.uint8)
    for i, b in enumerate(blinds):
        blind_rows[i] = np.frombuffer(b, dtype=np.uint8).reshape(t, 32)
    states = np.stack([np.frombuffer(tr.state, dtype=np.uint8) for tr in trs])
    d = dict(proofs=proofs, lens=lens, m=np.array(ms, dtype=np.uint32), commitments=commitments, min_values=min_values,
             min_present=min_present, seeds=seeds, seed_present=(np.array(ms) == 1).astype(np.uint8), blinds=blind_rows, states=states)
    for a in d.values():
        a.setflags(write=False)
    d["statements"], d["opened"], d["form"] = sts, opened, ("packed" if all(m == 1 for m in ms) else "mixed")
    return d


@pytest.fixture(scope="module")
def corpora(bpp, engine):
    """name -> (params, rows): "PA" / "PB" (packed, m = 1), "MA" / "MB" (mixed), 70 slots at t = 1; "T2": 9 mixed slots at t = 2"""
    made, params_of = {}, {}

    def get(name):
        if name not in made:
            t, count = (2, N2) if name == "T2" else (1, N)
            if t not in params_of:
                params_of[t] = bpp.RangeParameters.init(32, 4, bpp.create_pedersen_gens_with_extension_degree(t), engine=engine)
            ms = [1] * count if name[0] == "P" else [PATTERN[i % 7] for i in range(count)]
            made[name] = (params_of[t], _prove(bpp, params_of[t], 32, t, ms, name.encode()))
        return made[name]

    yield get
    for p in params_of.values():
        p.close()


def _with(d, **changed):
    out = dict(d)
    out.update(changed)
    return out


def _dev(a):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:
        a = a.copy()
    if a.dtype == np.uint64:
        a = a.view(np.int64)  # torch's uint64 is thin: the bit patterns travel as int64
    return torch.from_numpy(a).cuda()


def _dev_states(rows, offset=0):
    """the rows as a uint8 [n, 203] device tensor that starts `offset` bytes into a larger one"""
    rows = np.ascontiguousarray(rows)
    n = rows.shape[0]
    big = torch.full((n * 203 + 8,), 0xEE, dtype=torch.uint8, device="cuda")
    big[offset:offset + n * 203] = torch.from_numpy(rows.reshape(-1).copy()).cuda()
    view = big[offset:offset + n * 203].view(n, 203)
    assert view.data_ptr() % 4 == (big.data_ptr() + offset) % 4
    return view


def _input(packed, d, slots=slice(None), states="own", offset=0, state=None):
    """the rows at `slots`, in that order, as a device input of the corpus' form.  states: "own" (the rows' own transcripts), an array
    [n, 203], or None (no per-item transcripts: the existing uploads, under `state`)"""
    rows = d["states"][slots] if isinstance(states, str) else states
    kw = dict(item_states=_dev_states(rows, offset)) if rows is not None else dict(state=state)
    if d["form"] == "packed":
        ln = int(d["lens"][0])
        inp = packed.DevicePackedInput(_dev(d["proofs"][slots][:, :ln]), _dev(d["commitments"][slots][:, :1]), _dev(d["min_values"][slots][:, :1]),
                                       _dev(d["min_present"][slots][:, :1]), _dev(d["seeds"][slots]), b"", **kw)
    else:
        inp = packed.DeviceMixedInput(_dev(d["proofs"][slots]), d["lens"][slots].copy(), d["m"][slots].copy(), _dev(d["commitments"][slots]),
                                      _dev(d["min_values"][slots]), _dev(d["min_present"][slots]), _dev(d["seeds"][slots]), b"",
                                      seed_present=_dev(d["seed_present"][slots]), **kw)
    torch.cuda.synchronize()
    return inp


def _upload(packed, params, inp):
    if isinstance(inp, packed.DeviceMixedInput):
        return packed.ResidentBatch.from_mixed(params, inp)
    return packed.ResidentBatch(params, inp, None, None, None, None, b"", form="device")


def _item_batch(bpp, d, slots=slice(None), states="own"):
    """bpp_batch_upload on the equivalent item array: item k = the row at slots[k] under transcript_state = its state row"""
    idx = np.arange(len(d["lens"]))[slots]
    rows = d["states"][slots] if isinstance(states, str) else states
    trs = [bpp.Transcript.from_state(rows[k].tobytes()) for k in range(len(idx))]
    return bpp.ResidentBatch(trs, [d["statements"][i] for i in idx], [d["proofs"][i, :int(d["lens"][i])].tobytes() for i in idx])


def _actions(bpp):
    V, RV = int(bpp.VerifyAction.VerifyOnly), int(bpp.VerifyAction.RecoverAndVerify)
    return [RV, V, RV]


def _outputs(e, n, t=1):
    """(verdicts, masks, present, state rows or None) on the host"""
    e.wait()
    rows = None if e.states is None else e.states.cpu().numpy().copy()
    if e.masks is None:
        return (e.verdicts.cpu().numpy().copy(), np.zeros((n, t, 32), dtype=np.uint8), np.zeros(n, dtype=np.uint8), rows)
    return (e.verdicts.cpu().numpy().copy(), e.masks.cpu().numpy().copy(), e.present.cpu().numpy().copy(), rows)


def _mask(live=(), dead=None, n=N):
    mk = np.zeros(n, dtype=np.uint8) if dead is None else np.ones(n, dtype=np.uint8)
    for s in (live if dead is None else dead):
        mk[s] = 0 if dead is not None else 1
    return mk


def _mask_dev(mk):
    t = torch.from_numpy(np.ascontiguousarray(mk).copy()).cuda()
    torch.cuda.synchronize()
    return t


def _count_word(c):
    w = torch.tensor([c], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return w


def _groups(bounds, mk):
    slots = np.flatnonzero(mk)
    return [slots[(slots >= p0) & (slots < p1)] for p0, p1 in zip(bounds[:-1], bounds[1:])]


def _reference(packed, params, d, mk, bounds, actions, states="own"):
    """a fresh upload WITH TRANSCRIPTS of the live rows alone, the boundaries mapped and empty groups dropped, and
    bpp_verify_enqueue_states on it: (verdicts, masks, present, state rows), the last three in compacted order"""
    slots = np.flatnonzero(mk)
    cb, acts = [0], []
    for g, s in enumerate(_groups(bounds, mk)):
        if len(s):
            cb.append(cb[-1] + len(s))
            acts.append(actions[g])
    rows = d["states"][slots] if isinstance(states, str) else states[slots]
    rb = _upload(packed, params, _input(packed, d, slots, states=rows))
    try:
        return _outputs(rb.enqueue(bounds=cb, actions=acts, states=True), len(slots), rb.t)
    finally:
        rb.close()


@pytest.fixture(scope="module")
def references(bpp, packed, corpora):
    """(corpus name, mask) -> the reference of the clean corpus under the mask, made on first use and never changed"""
    made = {}

    def get(name, mk):
        key = (name, (mk != 0).tobytes())
        if key not in made:
            params, d = corpora(name)
            one = name == "T2"
            made[key] = _reference(packed, params, d, mk, [0, N2] if one else BOUNDS, [_actions(bpp)[0]] if one else _actions(bpp))
        return made[key]

    return get


def _empty_record(packed):
    return np.array([0, 0, 0, packed.VERDICT_WRITTEN | packed.VERDICT_EMPTY], dtype=np.int32)


def _hold(packed, got, want, bounds, mk, what):
    """records of non-empty groups -- the reference's, `index` mapped to the slot offset --, mask rows, mask_present and state rows of
    live slots: the reference's bytes; EMPTY records and zeros for the rest"""
    verdicts, masks, present, rows = got
    live = mk != 0
    k = 0
    for g, slots in enumerate(_groups(bounds, mk)):
        if not len(slots):
            assert (verdicts[g] == _empty_record(packed)).all(), (what, g, verdicts)
            continue
        w = want[0][k].copy()
        if w[3] == packed.VERDICT_WRITTEN and 2 <= w[1] <= 6:
            w[2] = slots[w[2]] - bounds[g]
        assert verdicts[g].tolist() == w.tolist(), (what, g, verdicts, want[0])
        k += 1
    if live.any():
        assert k == len(want[0])
        assert masks[live].tobytes() == want[1].tobytes(), (what, "masks")
        assert present[live].tobytes() == want[2].tobytes(), (what, "present")
        if rows is not None:
            assert rows[live].tobytes() == want[3].tobytes(), (what, "state rows")
    assert not masks[~live].any() and not present[~live].any(), (what, "dead slots")
    if rows is not None:
        assert not rows[~live].any(), (what, "state rows of dead slots")


def _all_ok(packed, verdicts):
    return (verdicts[:, :3] == 0).all() and (verdicts[:, 3] == packed.VERDICT_WRITTEN).all()


def _secret_bytes(eng, handle=0):
    k = ctypes.c_uint64()
    assert eng.lib.bpp_batch_secret_bytes(eng.ctx, handle, ctypes.byref(k)) == 0
    return k.value


ALL = _mask(dead=[])


def test_the_corpus_rows_differ_in_pos(corpora):
    for name in ("PA", "MA"):
        _, d = corpora(name)
        pos = d["states"][:, 200]
        assert pos[POS_SLOT] == STROBE_R - 1 and len(set(pos.tolist())) >= 40 and (pos < STROBE_R).all()
        assert len({r.tobytes() for r in d["states"]}) == N


# ---- (a) an upload with transcripts equals the item form: shape, traces, verdicts, masks
@pytest.mark.parametrize("name", ["PA", "MA", "T2"])
def test_upload_with_transcripts_equals_the_item_form(bpp, packed, corpora, opt, name):
    params, d = corpora(name)
    n = len(d["lens"])
    bounds, actions = ([0, N2], [_actions(bpp)[0]]) if name == "T2" else (BOUNDS, _actions(bpp))
    for wave in WAVES:
        opt("transcripts_wave", wave)
        dev, item = _upload(packed, params, _input(packed, d)), _item_batch(bpp, d)
        try:
            assert dev.shape() == item.shape()
            got = packed.verify_groups_actions(dev, bounds, actions)
            want = packed.verify_groups_actions(item, bounds, actions)
            assert got[0] == want[0] and all(r["code"] == 0 for r in got[0]), got[0]
            assert got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes() and got[2].any()
            for what in range(1, 8):
                assert dev.trace(what) == item.trace(what), (name, wave, what)
            e_dev = _outputs(dev.enqueue(bounds=bounds, actions=actions), n, dev.t)
            e_item = _outputs(packed.ResidentBatch.enqueue(item, bounds=bounds, actions=actions), n, dev.t)
            assert _all_ok(packed, e_dev[0])
            for a, b in zip(e_dev[:3], e_item[:3]):
                assert a.tobytes() == b.tobytes(), (name, wave)
            assert e_dev[1][e_dev[2] != 0].tobytes() == d["blinds"][e_dev[2] != 0].tobytes()
        finally:
            dev.close()
            item.close()


def test_the_staged_fall_back_takes_the_rows_along(bpp, packed, corpora, engine):
    """a first byte that disagrees: the batch is staged, state rows and all, and goes through the item form"""
    params, d = corpora("PA")
    pr = d["proofs"].copy()
    pr[7, 0] = 2
    t = _with(d, proofs=pr)
    rows = d["states"].copy()
    rows[3, 200] = 255  # (a bad state at a lower index: the item form's finding there, which the staged rows carry)
    for states, text in ((d["states"], None), (rows, "transcript state has pos >= rate")):
        before = packed.ingest_stats(engine)
        with pytest.raises(bpp.ProofError) as want:  # (a t = 1 proof read under another first byte does not parse)
            _item_batch(bpp, t, states=states).close()
        with pytest.raises(bpp.ProofError) as got:
            _upload(packed, params, _input(packed, t, states=states, offset=1)).close()
        after = packed.ingest_stats(engine)
        assert after[1] == before[1] + 1 and after[0] == before[0] and after[2] - before[2] >= N * 203
        assert got.value.kind == want.value.kind and got.value.msg == want.value.msg, (got.value, want.value)
        assert text is None or text in got.value.msg


# ---- (b) the rows matter: two rows swapped
@pytest.mark.parametrize("name", ["PA", "MA"])
def test_swapped_rows_reject_exactly_their_groups(bpp, packed, corpora, opt, name):
    params, d = corpora(name)
    rows = d["states"].copy()
    rows[[2, 40]] = rows[[40, 2]]
    actions = _actions(bpp)
    for wave in WAVES:
        opt("transcripts_wave", wave)
        dev, item = _upload(packed, params, _input(packed, d, states=rows)), _item_batch(bpp, d, states=rows)
        try:
            got = _outputs(dev.enqueue(bounds=BOUNDS, actions=actions), N)
            want = _outputs(packed.ResidentBatch.enqueue(item, bounds=BOUNDS, actions=actions), N)
            assert got[0].tolist() == want[0].tolist()
            assert got[0][0, 0] != 0 and got[0][2, 0] != 0 and got[0][1].tolist() == [0, 0, 0, packed.VERDICT_WRITTEN], got[0]
            assert got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes()
            assert packed.verify_groups(dev, BOUNDS) == packed.verify_groups(item, BOUNDS)
        finally:
            dev.close()
            item.close()


# ---- (c) all rows equal: the existing _device upload under that transcript_state
@pytest.mark.parametrize("name", ["PA", "MA"])
def test_equal_rows_are_the_one_transcript_of_the_device_upload(bpp, packed, corpora, opt, name):
    params, d = corpora(name)
    one = d["states"][3]
    rows = np.repeat(one[None, :], N, axis=0)
    bounds, actions = [0, 3, 4, 33, 70], _actions(bpp) + [int(bpp.VerifyAction.VerifyOnly)]
    for wave in WAVES:
        opt("transcripts_wave", wave)
        dev, old = _upload(packed, params, _input(packed, d, states=rows)), _upload(packed, params, _input(packed, d, states=None, state=one.tobytes()))
        try:
            got = _outputs(dev.enqueue(bounds=bounds, actions=actions), N)
            want = _outputs(old.enqueue(bounds=bounds, actions=actions), N)
            for a, b in zip(got[:3], want[:3]):
                assert a.tobytes() == b.tobytes()
            # only the group that holds slot 3 alone is valid under its transcript
            assert [int(c != 0) for c in got[0][:, 0]] == [1, 0, 1, 1], got[0]
        finally:
            dev.close()
            old.close()


# ---- (d) refills: plain, with a count, under a mask; new proofs and new transcripts each
@pytest.mark.parametrize("pair", [("PA", "PB"), ("MA", "MB")])
def test_plain_refill_equals_a_fresh_upload_with_transcripts(bpp, packed, corpora, references, opt, pair):
    params, a = corpora(pair[0])
    _, b = corpora(pair[1])
    assert a["states"].tobytes() != b["states"].tobytes()
    actions = _actions(bpp)
    rb = _upload(packed, params, _input(packed, a))
    try:
        for step, (name, d) in enumerate([(pair[1], b), (pair[0], a), (pair[1], b), (pair[0], a)]):
            opt("transcripts_wave", step % 2)
            filled = rb.refill(_input(packed, d, offset=step % 4))  # (e) the rows at every byte offset
            got = _outputs(rb.enqueue(bounds=BOUNDS, actions=actions, states=True), N)
            rec = filled.result()
            assert rec["flags"] == packed.REFILL_WRITTEN and rec["code"] == 0 and rec["msg"] == "", (name, rec)
            want = references(name, ALL)
            assert _all_ok(packed, want[0]) and want[3].any(axis=1).all()
            _hold(packed, got, want, BOUNDS, ALL, (name, step))
        with pytest.raises(bpp.ProofError):  # a refilled batch takes enqueued calls only
            rb.verify_only()
    finally:
        rb.close()


@pytest.mark.parametrize("pair", [("PA", "PB"), ("MA", "MB")])
@pytest.mark.parametrize("c", [0, 1, 5, 6, 64, 65, 70, 71])
def test_count_refill_equals_a_fresh_upload_of_the_first_rows(bpp, packed, corpora, references, opt, pair, c):
    params, a = corpora(pair[0])
    _, b = corpora(pair[1])
    actions = _actions(bpp)
    rb = _upload(packed, params, _input(packed, a))
    try:
        # the source ends behind the last live row: rows at and beyond the count do not exist
        k = min(c, N) if c <= N else 0
        rows = np.concatenate([b["states"][:k], np.full((N - k, 203), 0xFF, dtype=np.uint8)])
        for wave in WAVES:
            opt("transcripts_wave", wave)
            filled = rb.refill(_input(packed, b, states=rows, offset=1 + wave), count=_count_word(c))
            got = _outputs(rb.enqueue(bounds=BOUNDS, actions=actions, states=True), N)
            rec = filled.result()
            if c > N:
                assert rec["flags"] == packed.REFILL_WRITTEN | packed.REFILL_COUNT and rec["code"] == 0, rec
                assert (got[0] == np.array([0, 0, 0, packed.VERDICT_WRITTEN | packed.VERDICT_REFILL], dtype=np.int32)).all(), got[0]
                assert not got[1].any() and not got[2].any() and not got[3].any()
                continue
            assert rec["flags"] == packed.REFILL_WRITTEN and rec["code"] == 0, rec
            mk = _mask([slice(0, c)])
            _hold(packed, got, references(pair[1], mk) if c else None, BOUNDS, mk, ("count", c, wave))
    finally:
        rb.close()


MASKS = [("all live", ALL), ("all dead", _mask()), ("only slot 0", _mask([0])), ("only slot 69", _mask([69])),
         ("every other slot", _mask([slice(0, N, 2)])), ("group [5, 33) dead", _mask(dead=[slice(5, 33)])),
         ("random", (np.random.default_rng(101).random(N) < 0.5).astype(np.uint8))]


@pytest.mark.parametrize("pair", [("PA", "PB"), ("MA", "MB")])
def test_every_mask_equals_a_fresh_upload_of_the_live_rows(bpp, packed, corpora, references, opt, pair):
    params, a = corpora(pair[0])
    _, b = corpora(pair[1])
    actions = _actions(bpp)
    rb = _upload(packed, params, _input(packed, a))
    try:
        for i, (name, mk) in enumerate(MASKS + MASKS[::-1]):
            opt("transcripts_wave", (i // 2) % 2)
            which = pair[1] if i % 2 == 0 else pair[0]
            d = b if i % 2 == 0 else a
            # dead rows hold a state that would be a finding: nothing of them is read
            rows = d["states"].copy()
            rows[mk == 0] = 0xFF
            loud = mk * np.where(np.arange(N) % 2 == 0, 2, 255).astype(np.uint8)
            filled = rb.refill(_input(packed, d, states=rows, offset=i % 4), live=_mask_dev(loud))
            got = _outputs(rb.enqueue(bounds=BOUNDS, actions=actions, states=True), N)
            rec = filled.result()
            assert rec["flags"] == packed.REFILL_WRITTEN and rec["code"] == 0, (name, rec)
            _hold(packed, got, references(which, mk) if mk.any() else None, BOUNDS, mk, (name, which))
    finally:
        rb.close()


def test_t2_refill_and_rows(bpp, packed, corpora, references, opt):
    params, d = corpora("T2")
    RV = int(bpp.VerifyAction.RecoverAndVerify)
    rb = _upload(packed, params, _input(packed, d))
    try:
        for wave, mk in zip((0, 1, 0), (_mask([1, 3, 4, 8], n=N2), _mask(dead=[], n=N2), _mask([slice(0, 5)], n=N2))):
            opt("transcripts_wave", wave)
            if mk[:5].all() and not mk[5:].any():
                rb.refill(_input(packed, d, offset=3), count=_count_word(5))
            else:
                rb.refill(_input(packed, d, offset=2), live=_mask_dev(mk))
            got = _outputs(rb.enqueue(actions=[RV], states=True), N2, 2)
            want = references("T2", mk)
            assert _all_ok(packed, want[0]) and got[2].any()
            _hold(packed, got, want, [0, N2], mk, "t = 2")
    finally:
        rb.close()


# ---- (f) bad states: pos 166 and 255, alone and with a non-canonical scalar
def _bad(d, state_at=(), scalar_at=None):
    rows, pr = d["states"].copy(), d["proofs"].copy()
    for i, pos in state_at:
        rows[i, 200] = pos
    if scalar_at is not None:
        pr[scalar_at, D1:D1 + 32] = L_BYTES
    return _with(d, proofs=pr), rows


BAD_CASES = [("the first slot", dict(state_at=[(0, 166)]), 0), ("the last slot", dict(state_at=[(69, 255)]), 69),
             ("two bad rows", dict(state_at=[(37, 255), (13, 166)]), 13),
             ("a bad scalar at the same index wins", dict(state_at=[(36, 166)], scalar_at=36), 36),
             ("a bad scalar at a higher index loses", dict(state_at=[(36, 166)], scalar_at=50), 36),
             ("a bad scalar at a lower index wins", dict(state_at=[(36, 255)], scalar_at=8), 8)]


@pytest.mark.parametrize("name", ["PA", "MA"])
def test_bad_states_at_upload_are_the_item_forms_finding(bpp, packed, corpora, name):
    params, d = corpora(name)
    for what, how, index in BAD_CASES:
        t, rows = _bad(d, **how)
        with pytest.raises(bpp.ProofError) as want:
            _item_batch(bpp, t, states=rows).close()
        with pytest.raises(bpp.ProofError) as got:
            _upload(packed, params, _input(packed, t, states=rows, offset=3)).close()
        assert got.value.kind == want.value.kind and got.value.msg == want.value.msg, (what, got.value, want.value)
        scalar_wins = how.get("scalar_at") == index
        assert ("transcript state has pos >= rate" in got.value.msg) == (not scalar_wins), (what, got.value.msg)
    # one item alone
    rows = d["states"][:1].copy()
    rows[0, 200] = 166
    with pytest.raises(bpp.ProofError) as got:
        _upload(packed, params, _input(packed, d, slice(0, 1), states=rows)).close()
    assert "transcript state has pos >= rate" in got.value.msg


@pytest.mark.parametrize("pair", [("PA", "PB"), ("MA", "MB")])
def test_bad_states_at_refill_land_in_the_record(bpp, packed, corpora, references, opt, pair):
    params, a = corpora(pair[0])
    _, b = corpora(pair[1])
    actions = _actions(bpp)
    F = _mask(dead=[slice(6, 33, 3), 40, 47, 69])
    assert F[[0, 13, 36, 37, 50, 8]].all() and not F[[9, 40, 69]].any()
    live = _mask_dev(F)
    refill_flag = packed.VERDICT_WRITTEN | packed.VERDICT_REFILL
    rb = _upload(packed, params, _input(packed, a))

    def refused(t, rows, mk):
        """what the fresh upload with transcripts of the live rows throws, which is what the item form throws"""
        slots = np.flatnonzero(mk)
        with pytest.raises(bpp.ProofError) as dev:
            _upload(packed, params, _input(packed, t, slots, states=rows[slots])).close()
        with pytest.raises(bpp.ProofError) as item:
            _item_batch(bpp, t, slots, states=rows[slots]).close()
        assert dev.value.kind == item.value.kind and dev.value.msg == item.value.msg
        return dev.value

    try:
        for step, (what, how, index) in enumerate(BAD_CASES):
            t, rows = _bad(b, **how)
            for mk, kw in ((F, dict(live=live)), (ALL, dict())):
                if not mk[index]:
                    continue
                opt("transcripts_wave", step % 2)
                filled = rb.refill(_input(packed, t, states=rows, offset=step % 4), **kw)
                got = _outputs(rb.enqueue(bounds=BOUNDS, actions=actions, states=True), N)
                rec, err = filled.result(), refused(t, rows, mk)
                assert rec["flags"] == packed.REFILL_WRITTEN | packed.REFILL_FINDING and rec["index"] == index and rec["tier"] == 1, (what, rec)
                assert rec["code"] == int(err.kind) and rec["msg"] == err.msg, (what, rec, err)
                want = np.array([rec["code"], 1, index, refill_flag], dtype=np.int32)
                assert (got[0] == want).all() and not got[1].any() and not got[2].any() and not got[3].any(), (what, got[0])
        # bad states at dead slots, under a mask and beyond a count: no finding -- exactly the clean rows
        t, rows = _bad(b, state_at=[(9, 166), (40, 255), (69, 166)])
        assert rb.refill(_input(packed, t, states=rows), live=live).result()["flags"] == packed.REFILL_WRITTEN
        _hold(packed, _outputs(rb.enqueue(bounds=BOUNDS, actions=actions, states=True), N), references(pair[1], F), BOUNDS, F, "bad states at dead slots")
        assert rb.refill(_input(packed, t, states=rows), count=_count_word(9)).result()["flags"] == packed.REFILL_WRITTEN
        mk = _mask([slice(0, 9)])
        _hold(packed, _outputs(rb.enqueue(bounds=BOUNDS, actions=actions, states=True), N), references(pair[1], mk), BOUNDS, mk, "bad states beyond the count")
    finally:
        rb.close()


# ---- (g) states out
@pytest.mark.parametrize("name", ["PA", "MA", "T2"])
def test_states_out_are_those_of_the_blocking_form(bpp, packed, corpora, opt, name):
    params, d = corpora(name)
    n = len(d["lens"])
    bounds, actions = ([0, 4, N2], _actions(bpp)[:2]) if name == "T2" else (BOUNDS, _actions(bpp))
    # the rows bpp_verify_batch_states writes, group by group (each group is one reference batch)
    want = np.zeros((n, 203), dtype=np.uint8)
    for p0, p1 in zip(bounds[:-1], bounds[1:]):
        trs = [bpp.Transcript.from_state(d["states"][i].tobytes()) for i in range(p0, p1)]
        bpp.RangeProof.verify_batch(trs, d["statements"][p0:p1], [d["proofs"][i, :int(d["lens"][i])].tobytes() for i in range(p0, p1)],
                                    bpp.VerifyAction.VerifyOnly, chunk=0, advance=True)
        want[p0:p1] = np.stack([np.frombuffer(tr.state, dtype=np.uint8) for tr in trs])
    assert want.any(axis=1).all() and (want != d["states"]).any(axis=1).all()
    # a batch with one transcript per item, and the item form's batch (whose table is the de-duplicated one)
    dev, item = _upload(packed, params, _input(packed, d)), _item_batch(bpp, d)
    try:
        for wave in WAVES:
            opt("transcripts_wave", wave)
            for rb in (dev, item):
                plain = _outputs(packed.ResidentBatch.enqueue(rb, bounds=bounds, actions=actions), n, dev.t)
                big = torch.full((n * 203 + 4,), 0xEE, dtype=torch.uint8, device="cuda")
                out = big[1 + wave:1 + wave + n * 203].view(n, 203)  # the caller's array at an odd byte address
                got = _outputs(packed.ResidentBatch.enqueue(rb, bounds=bounds, actions=actions, states=out), n, dev.t)
                assert _all_ok(packed, got[0])
                for x, y in zip(got[:3], plain[:3]):
                    assert x.tobytes() == y.tobytes()
                assert got[3].tobytes() == want.tobytes(), (name, wave)
                edge = big.cpu().numpy()
                assert (edge[:1 + wave] == 0xEE).all() and (edge[1 + wave + n * 203:] == 0xEE).all()
    finally:
        dev.close()
        item.close()


def test_states_out_are_zero_where_nothing_is_claimed(bpp, packed, corpora, references, opt):
    params, a = corpora("PA")
    _, b = corpora("PB")
    actions = _actions(bpp)
    pr = a["proofs"].copy()
    pr[20, R1] ^= 1  # an invalid proof in group [5, 33)
    t = _with(a, proofs=pr)
    rb = _upload(packed, params, _input(packed, t))
    try:
        for wave in WAVES:
            opt("transcripts_wave", wave)
            plain = _outputs(rb.enqueue(bounds=BOUNDS, actions=actions), N)
            got = _outputs(rb.enqueue(bounds=BOUNDS, actions=actions, states=True), N)
            for x, y in zip(got[:3], plain[:3]):
                assert x.tobytes() == y.tobytes()
            assert got[0][1, 0] != 0 and got[0][0, 0] == 0 and got[0][2, 0] == 0, got[0]
            assert not got[3][5:33].any() and got[3][:5].any(axis=1).all() and got[3][33:].any(axis=1).all()
            want = references("PA", ALL)  # (the clean corpus: the rows of the groups that hold no tampered proof)
            assert got[3][:5].tobytes() == want[3][:5].tobytes() and got[3][33:].tobytes() == want[3][33:].tobytes()
        # an EMPTY group and dead slots
        mk = _mask(dead=[slice(5, 33), 2, 69])
        rb.refill(_input(packed, b), live=_mask_dev(mk))
        got = _outputs(rb.enqueue(bounds=BOUNDS, actions=actions, states=True), N)
        assert (got[0][1] == _empty_record(packed)).all()
        _hold(packed, got, references("PB", mk), BOUNDS, mk, "an empty group")
        assert got[3][mk != 0].any(axis=1).all()
        # a refill that did not take: no row
        foreign = b["proofs"].copy()
        foreign[11, 0] = 2
        rec = rb.refill(_input(packed, _with(b, proofs=foreign))).result()
        assert rec["flags"] == packed.REFILL_WRITTEN | packed.REFILL_FALLBACK, rec
        got = _outputs(rb.enqueue(bounds=BOUNDS, actions=actions, states=True), N)
        assert (got[0][:, 3] == (packed.VERDICT_WRITTEN | packed.VERDICT_REFILL)).all() and not got[3].any()
    finally:
        rb.close()


def test_a_returned_row_continues_like_the_oracles_merlin(bpp, packed, corpora):
    """one item: the oracle replays the verifier on its own Merlin transcript; a challenge drawn afterwards is the same on both sides"""
    params, d = corpora("PA")
    i = POS_SLOT
    vals, bl, mins, nonce = d["opened"][i]
    o_params = O.RangeParameters(32, 1, O.PedersenGens(1))
    blind = [int.from_bytes(x, "little") for x in bl[0]]
    comm = o_params.pc_gens.commit(vals[0], blind)
    o_st = O.RangeStatement(o_params, [comm], mins, int.from_bytes(nonce, "little"))
    o_tr = M.Transcript(LABEL)
    length = _length_for_pos(bpp, STROBE_R - 1)
    unit = b"PA/%d/" % i
    o_tr.append_message(CTX_LABEL, (unit * (length // len(unit) + 1))[:length])
    assert o_tr.strobe.to_bytes() == d["states"][i].tobytes()
    O.verify([o_tr], [o_st], [O.RangeProof.from_bytes(d["proofs"][i, :int(d["lens"][i])].tobytes())], 0)
    rb = _upload(packed, params, _input(packed, d, slice(i, i + 1)))
    try:
        got = _outputs(rb.enqueue(states=True), 1)
        assert _all_ok(packed, got[0])
        row = got[3][0].tobytes()
        assert row == o_tr.strobe.to_bytes()
        assert bpp.Transcript.from_state(row).challenge_bytes(b"after", 32) == o_tr.challenge_bytes(b"after", 32)
    finally:
        rb.close()


# ---- (h) refusals before any launch
def test_refusals_before_any_launch(bpp, packed, corpora, engine, opt):
    K = bpp.ProofErrorKind
    lib, eng = packed._lib, engine
    err = ctypes.create_string_buffer(256)
    label = np.frombuffer(LABEL, dtype=np.uint8).copy()
    for name in ("PA", "MA"):
        params, d = corpora(name)
        mixed = d["form"] == "mixed"
        inp, plain_inp = _input(packed, d), _input(packed, d, states=None)
        with_rb, without_rb = _upload(packed, params, inp), _upload(packed, params, plain_inp)
        Struct = lib.MixedBatch if mixed else lib.PackedBatch
        upload = eng.lib.bpp_batch_upload_mixed_device_transcripts if mixed else eng.lib.bpp_batch_upload_packed_device_transcripts
        refill = eng.lib.bpp_batch_refill_enqueue_mixed_transcripts if mixed else eng.lib.bpp_batch_refill_enqueue_transcripts
        host_rows = d["states"].copy()
        rows_dev = inp.item_states
        verdicts = torch.empty((3, 4), dtype=torch.int32, device="cuda")
        out = torch.empty((N, 203), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def struct(**fields):
            st = Struct.from_buffer_copy(inp.struct_without_transcript())
            for k, v in fields.items():
                setattr(st, k, v)
            return st

        def up(st, rows):
            h = ctypes.c_uint64()
            rc = upload(eng.ctx, params.handle, ctypes.byref(st), rows, ctypes.byref(h), err, 256)
            return rc, err.value.decode()

        def re(rb, st, rows, count=None, live=None):
            rc = refill(eng.ctx, rb.handle, ctypes.byref(st), rows, count, live, None, None)
            return rc, eng.lib.bpp_ctx_last_error(eng.ctx).decode()

        def enq(rb, states, bounds=BOUNDS):
            arr = (ctypes.c_uint32 * len(bounds))(*bounds)
            tk = ctypes.c_uint64()
            rc = eng.lib.bpp_verify_enqueue_states(eng.ctx, rb.handle, arr, len(bounds) - 1, 0, None, 0, ctypes.c_void_p(verdicts.data_ptr()), None, None,
                                                   states, ctypes.byref(tk))
            return rc, eng.lib.bpp_ctx_last_error(eng.ctx).decode()

        try:
            before = (packed.refill_stats(eng), packed.enqueue_stats(eng), packed.ingest_stats(eng))
            checks = [
                (up(struct(), None), "item_states203 is null"),
                (up(struct(), ctypes.c_void_p(host_rows.ctypes.data)), "item_states203 is not device memory"),
                (up(struct(transcript_state=label.ctypes.data), rows_dev), "transcript_state must be null"),
                (up(struct(transcript_label=label.ctypes.data, label_len=len(LABEL)), rows_dev), "transcript_label must be null"),
                (re(with_rb, struct(), None), "item_states203_dev is null"),
                (re(with_rb, struct(), ctypes.c_void_p(host_rows.ctypes.data)), "item_states203_dev: not device memory"),
                (re(with_rb, struct(transcript_state=label.ctypes.data), rows_dev), "transcript_state / transcript_label must be null"),
                (re(with_rb, struct(), rows_dev, count=ctypes.c_void_p(_count_word(3).data_ptr()), live=ctypes.c_void_p(_mask_dev(ALL).data_ptr())),
                 "count_dev and live_dev"),
                # the wrong kind of batch, in both directions: the text names the call to use instead
                (re(without_rb, struct(), rows_dev), "use bpp_batch_refill_enqueue" + ("_mixed" if mixed else " / _count / _live")),
                (enq(with_rb, None), "states_out203_dev is null"),
                (enq(with_rb, ctypes.c_void_p(host_rows.ctypes.data)), "states_out203_dev: not device memory"),
            ]
            for (rc, msg), text in checks:
                assert rc == int(K.InvalidArgument) and text in msg, (name, text, rc, msg)
            with pytest.raises(bpp.ProofError) as e:
                with_rb.refill(plain_inp)  # (an input without rows reaches the existing refills)
            assert "per-item transcripts" in e.value.msg and ("bpp_batch_refill_enqueue_mixed_transcripts" if mixed else "bpp_batch_refill_enqueue_transcripts") in e.value.msg
            opt("verify_check", 1)
            rc, msg = enq(with_rb, ctypes.c_void_p(out.data_ptr()))
            assert rc == int(K.InvalidArgument) and "verify_check" in msg, msg
            opt("verify_check", -1)
            assert (packed.refill_stats(eng), packed.enqueue_stats(eng), packed.ingest_stats(eng)) == before
            with_rb.verify_only()  # nothing was launched: the batch is still the host's
        finally:
            torch.cuda.synchronize()
            with_rb.close()
            without_rb.close()


# ---- (i) the steady state and the secrets
@pytest.mark.parametrize("pair", [("PA", "PB"), ("MA", "MB")])
def test_steady_state_and_secrets(bpp, packed, corpora, references, pair):
    _, a = corpora(pair[0])
    _, b = corpora(pair[1])
    actions = _actions(bpp)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        eng = bpp.Engine(0, stream=stream.cuda_stream)
        params = bpp.RangeParameters.init(32, 4, bpp.create_pedersen_gens_with_extension_degree(1), engine=eng)
        inputs = {pair[0]: _input(packed, a), pair[1]: _input(packed, b, offset=1)}
        rb = _upload(packed, params, inputs[pair[0]])
        masks = [m for _, m in MASKS if m.any()]
        dev_masks = [_mask_dev(m) for m in masks]
        try:
            rb.refill(inputs[pair[1]]).result()  # the first refill: the batch's words
            rb.enqueue(bounds=BOUNDS, actions=actions, states=True).wait()  # the layout and the row buffer, with nothing in flight
            rb.refill(inputs[pair[0]], live=dev_masks[0]).result()  # the first mask
            r1, e1 = packed.refill_stats(eng), packed.enqueue_stats(eng)
            runs = []
            for step in range(8):
                which = pair[step % 2]
                k = step % len(masks)
                rb.refill(inputs[which], live=dev_masks[k])
                runs.append((which, masks[k], rb.enqueue(bounds=BOUNDS, actions=actions, states=True)))
            r2, e2 = packed.refill_stats(eng), packed.enqueue_stats(eng)  # (before any wait)
            assert r2["host_waits"] == 0 and e2["host_waits"] == e1["host_waits"] == 0
            assert r2["calls"] == r1["calls"] + 8 and e2["calls"] == e1["calls"] + 8
            assert e2["layouts_in_call"] == e1["layouts_in_call"] and r2["first_calls"] == r1["first_calls"]
            for which, mk, e in runs:
                _hold(packed, _outputs(e, N), references(which, mk), BOUNDS, mk, ("steady", which))
            # secrets: the nonces of the live nonce-bearing slots, and none once no such slot is live
            some = _mask([slice(0, 40)])
            rb.refill(inputs[pair[0]], live=_mask_dev(some))
            assert _secret_bytes(eng, rb.handle) == np.count_nonzero(a["seeds"][(some != 0) & (a["seed_present"] != 0)]) > 0
            rb.refill(inputs[pair[1]], live=_mask_dev(np.zeros(N, dtype=np.uint8)))
            assert _secret_bytes(eng, rb.handle) == 0
            rb.close()
            assert _secret_bytes(eng) == 0
        finally:
            torch.cuda.synchronize()
            rb.close()
            params.close()
            eng.close()
