"""GPU tests: a resident batch of MIXED aggregation factors is refilled on the stream (bpp_batch_refill_enqueue_mixed,
csrc/refill.h in its mixed form), plain, with a live count and under a per-item live mask.

The reference in every comparison is a FRESH bpp_batch_upload_mixed_device of the rows in question -- all of them, the first c, the
live ones alone in slot order, with the group boundaries mapped to the compacted rows and empty groups dropped -- plus
bpp_verify_enqueue: its records, masks and mask_present, and, for the weights, BPP_TRACE_WEIGHTS of a blocking call on that fresh
upload, scattered back to the slots.  A record's `index` is mapped from the reference's k-th live item of the group to that item's
slot offset.  A refilled batch is never compared with its own output.  References of the clean corpora are made once per (corpus,
mask) and shared.

The corpus: n_bits = 32, m_max = 4, t = 1, 70 slots in the pattern [4, 1, 2, 1, 1, 4, 2] -- four different items per wavefront of the
refill kernel, a partly filled last workgroup, one slot past the chain's 64-proof stage -- under the boundaries [0, 5, 33, 70]; two
corpora A and B of that shape vector; nonces on the m = 1 items, promises on every third opening.  A third corpus of 9 slots at t = 2
for the width of the mask rows."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from oracle.pyref import protocol as O
from tests.helpers import LABEL, Prng, sb

pytestmark = pytest.mark.gpu

L_BYTES = np.frombuffer(bytes.fromhex("edd3f55c1a631258d69cf7a2def9de14" + "00" * 15 + "10"), dtype=np.uint8)  # the group order
PATTERN = [4, 1, 2, 1, 1, 4, 2]
M_STRIDE = 8
SLACK = 40
N, BOUNDS = 70, [0, 5, 33, 70]
N2 = 9
D1, R1, S1 = 1, 1 + 32 * 4, 1 + 32 * 5  # t = 1: [t] d1 A A1 B r1 s1 (L R)*
MS = np.array([PATTERN[i % 7] for i in range(N)])


@pytest.fixture(scope="module")
def packed():
    return importlib.import_module("bulletproofs-plus_amd.packed")


def _prove(bpp, params, n_bits, t, count, seed):
    """rows of `count` items in the m pattern, proved by ONE bpp_prove_batch_mixed call"""
    rng = Prng(seed)
    ms = [PATTERN[i % 7] for i in range(count)]
    trs, sts, ws, exts, blinds = [], [], [], [], []
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
        trs.append(bpp.Transcript.new(LABEL))
        sts.append(bpp.RangeStatement.init(params, comms, mins, nonce))
        ws.append(bpp.RangeWitness.init([bpp.CommitmentOpening.new(vals[j], bl[j]) for j in range(m)]))
        exts.append(rng.fill_bytes(32 * (rounds + 3)))
        blinds.append(b"".join(bl[0]))
        commitments[i, :m] = np.frombuffer(b"".join(comms), dtype=np.uint8).reshape(m, 32)
        for j, v in enumerate(mins):
            if v is not None:
                min_values[i, j], min_present[i, j] = v, 1
        if nonce is not None:
            seeds[i] = np.frombuffer(nonce, dtype=np.uint8)
    raw = [g.to_bytes() for g in bpp.RangeProof.prove_batch_mixed(trs, sts, ws, exts)]
    lens = np.array([len(r) for r in raw], dtype=np.uintp)
    proofs = np.zeros((count, int(lens.max()) + SLACK), dtype=np.uint8)
    for i, r in enumerate(raw):
        proofs[i, :len(r)] = np.frombuffer(r, dtype=np.uint8)
    blind_rows = np.zeros((count, t, 32), dtype=np.uint8)
    for i, b in enumerate(blinds):
        blind_rows[i] = np.frombuffer(b, dtype=np.uint8).reshape(t, 32)
    d = dict(proofs=proofs, lens=lens, m=np.array(ms, dtype=np.uint32), commitments=commitments, min_values=min_values,
             min_present=min_present, seeds=seeds, seed_present=(np.array(ms) == 1).astype(np.uint8), blinds=blind_rows)
    for a in d.values():
        a.setflags(write=False)
    return d


@pytest.fixture(scope="module")
def corpora(bpp, engine):
    """name -> (params, rows): "A" and "B" (70 slots, t = 1, the same shape vector), "T2" (9 slots, t = 2); proved once, read-only"""
    made, params_of = {}, {}

    def get(name):
        if name not in made:
            t, count = (2, N2) if name == "T2" else (1, N)
            if t not in params_of:
                params_of[t] = bpp.RangeParameters.init(32, 4, bpp.create_pedersen_gens_with_extension_degree(t), engine=engine)
            made[name] = (params_of[t], _prove(bpp, params_of[t], 32, t, count, b"refill-mixed-" + name.encode()))
        return made[name]

    yield get
    for p in params_of.values():
        p.close()


def _with(d, **changed):
    """the rows with some arrays replaced (writable copies are the caller's business)"""
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


def _input(packed, d, slots=slice(None), pad=0, m_stride=M_STRIDE):
    """the rows at `slots`, in that order, as a DeviceMixedInput; pad / m_stride: another geometry of the same used bytes"""
    proofs = d["proofs"][slots]
    if pad:
        proofs = np.concatenate([proofs, np.full((proofs.shape[0], pad), 0xEE, dtype=np.uint8)], axis=1)
    inp = packed.DeviceMixedInput(_dev(proofs), d["lens"][slots].copy(), d["m"][slots].copy(), _dev(d["commitments"][slots][:, :m_stride]),
                                  _dev(d["min_values"][slots][:, :m_stride]), _dev(d["min_present"][slots][:, :m_stride]),
                                  _dev(d["seeds"][slots]), LABEL, seed_present=_dev(d["seed_present"][slots]))
    torch.cuda.synchronize()
    return inp


def _actions(bpp):
    V, RV = int(bpp.VerifyAction.VerifyOnly), int(bpp.VerifyAction.RecoverAndVerify)
    return [RV, V, RV]


def _outputs(e, n, t=1):
    """(verdicts, masks, present) on the host; a call in which no group recovers hands out no masks: zeros for `n` items"""
    e.wait()
    if e.masks is None:
        return (e.verdicts.cpu().numpy().copy(), np.zeros((n, t, 32), dtype=np.uint8), np.zeros(n, dtype=np.uint8))
    return (e.verdicts.cpu().numpy().copy(), e.masks.cpu().numpy().copy(), e.present.cpu().numpy().copy())


def _mask(live=(), dead=None, n=N):
    """ones at `live` (slots or slices); with `dead`: ones everywhere but there"""
    mk = np.zeros(n, dtype=np.uint8) if dead is None else np.ones(n, dtype=np.uint8)
    for s in (live if dead is None else dead):
        mk[s] = 0 if dead is not None else 1
    return mk


def _loud(mk):
    """the same mask with 2 and 255 for "live" """
    out = mk.copy()
    idx = np.flatnonzero(mk)
    out[idx[::2]] = 2
    out[idx[1::2]] = 255
    return out


def _mask_dev(mk):
    t = torch.from_numpy(np.ascontiguousarray(mk).copy()).cuda()
    torch.cuda.synchronize()  # (complete before any engine's stream reads it)
    return t


def _count_word(c):
    w = torch.tensor([c], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return w


def _groups(bounds, mk):
    """per group: the live slots in slot order"""
    slots = np.flatnonzero(mk)
    return [slots[(slots >= p0) & (slots < p1)] for p0, p1 in zip(bounds[:-1], bounds[1:])]


def _reference(packed, params, d, mk, bounds, actions, weights=True):
    """a fresh mixed device upload of the live rows alone, the boundaries mapped and empty groups dropped: (verdicts, masks, present,
    weights of a blocking call), the last three in compacted order"""
    slots = np.flatnonzero(mk)
    cb, acts = [0], []
    for g, s in enumerate(_groups(bounds, mk)):
        if len(s):
            cb.append(cb[-1] + len(s))
            acts.append(actions[g])
    rb = packed.ResidentBatch.from_mixed(params, _input(packed, d, slots))
    try:
        out = _outputs(rb.enqueue(bounds=cb, actions=acts), len(slots), rb.t)
        w = None
        if weights:
            packed.verify_groups(rb, cb)
            w = np.frombuffer(rb.trace(3), dtype=np.uint8).reshape(len(slots), 32).copy()
        return out + (w,)
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
            made[key] = _reference(packed, params, d, mk, BOUNDS if name != "T2" else [0, N2], _actions(bpp) if name != "T2" else [_actions(bpp)[0]])
        return made[key]

    return get


def _empty_record(packed):
    return np.array([0, 0, 0, packed.VERDICT_WRITTEN | packed.VERDICT_EMPTY], dtype=np.int32)


def _hold(packed, got, want, bounds, mk, what, weights=None):
    """records of non-empty groups -- the reference's, `index` mapped to the slot offset --, mask rows, mask_present and weights of live
    slots: the reference's bytes; EMPTY records and zeros for the rest"""
    verdicts, masks, present = got[:3]
    live = mk != 0
    k = 0
    for g, slots in enumerate(_groups(bounds, mk)):
        if not len(slots):
            assert (verdicts[g] == _empty_record(packed)).all(), (what, g, verdicts)
            continue
        w = want[0][k].copy()
        if w[3] == packed.VERDICT_WRITTEN and 2 <= w[1] <= 6:  # a finding at the reference's w[2]-th live item of the group
            w[2] = slots[w[2]] - bounds[g]
        assert verdicts[g].tolist() == w.tolist(), (what, g, verdicts, want[0])
        k += 1
    if live.any():
        assert k == len(want[0])
        assert masks[live].tobytes() == want[1].tobytes(), (what, "masks")
        assert present[live].tobytes() == want[2].tobytes(), (what, "present")
        if weights is not None:
            assert weights[live].tobytes() == want[3].tobytes(), (what, "weights")
            assert want[3].any(axis=1).all()
    assert not masks[~live].any() and not present[~live].any(), (what, "dead slots")
    if weights is not None:
        assert not weights[~live].any(), (what, "dead weights")


def _clean_and_recovered(bpp, packed, got, want, d, mk, actions, bounds, what):
    """valid proofs: every live group is Ok, and the masks are the openings' blinding factors where the group recovers and the slot has a nonce"""
    assert (want[0][:, :3] == 0).all() and (want[0][:, 3] == packed.VERDICT_WRITTEN).all(), (what, want[0])
    recovers = np.zeros(len(mk), dtype=bool)
    for g in range(len(bounds) - 1):
        if actions[g] != int(bpp.VerifyAction.VerifyOnly):
            recovers[bounds[g]:bounds[g + 1]] = True
    recovers &= (mk != 0) & (d["seed_present"] != 0)
    assert got[2].tolist() == recovers.astype(np.uint8).tolist(), what
    assert got[1][recovers].tobytes() == d["blinds"][recovers].tobytes(), what


def _secret_bytes(eng, handle=0):
    k = ctypes.c_uint64()
    assert eng.lib.bpp_batch_secret_bytes(eng.ctx, handle, ctypes.byref(k)) == 0
    return k.value


ALL = _mask(dead=[])


# ---- 1. the plain form: B into a batch of A and back, with and without the shape vectors, from rows of another geometry
def test_plain_refill_equals_a_fresh_upload(bpp, packed, corpora, references):
    params, a = corpora("A")
    _, b = corpora("B")
    assert (a["lens"] == b["lens"]).all() and (a["m"] == b["m"]).all() and a["proofs"].tobytes() != b["proofs"].tobytes()
    actions = _actions(bpp)
    rb = packed.ResidentBatch.from_mixed(params, _input(packed, a))
    try:
        steps = [("B", b, dict()), ("A", a, dict()), ("B", b, dict(shape_vectors=False)), ("A", a, dict(pad=24, m_stride=5)),
                 ("B", b, dict(pad=8, m_stride=4, shape_vectors=False))]
        for name, d, how in steps:
            kw = {k: how[k] for k in ("shape_vectors",) if k in how}
            inp = _input(packed, d, pad=how.get("pad", 0), m_stride=how.get("m_stride", M_STRIDE))
            filled = rb.refill(inp, **kw)
            got = _outputs(rb.enqueue(bounds=BOUNDS, actions=actions), N)
            weights = rb.enqueue_weights().numpy()
            rec = filled.result()
            assert rec["flags"] == packed.REFILL_WRITTEN and rec["code"] == 0 and rec["msg"] == "", (name, how, rec)
            want = references(name, ALL)
            _hold(packed, got, want, BOUNDS, ALL, (name, how), weights)
            _clean_and_recovered(bpp, packed, got, want, d, ALL, actions, BOUNDS, (name, how))
        # a refilled batch takes enqueued calls only
        with pytest.raises(bpp.ProofError):
            rb.verify_only()
    finally:
        rb.close()


# ---- 2. the live count
@pytest.mark.parametrize("c", [0, 1, 5, 6, 64, 65, 70, 71])
def test_count_refill_equals_a_fresh_upload_of_the_first_rows(bpp, packed, corpora, references, c):
    params, a = corpora("A")
    _, b = corpora("B")
    actions = _actions(bpp)
    rb = packed.ResidentBatch.from_mixed(params, _input(packed, a))
    try:
        filled = rb.refill(_input(packed, b), count=_count_word(c), shape_vectors=c % 2 == 0)
        got = _outputs(rb.enqueue(bounds=BOUNDS, actions=actions), N)
        weights = rb.enqueue_weights().numpy()
        rec = filled.result()
        if c > N:
            assert rec["flags"] == packed.REFILL_WRITTEN | packed.REFILL_COUNT and rec["code"] == 0 and rec["tier"] == 0 and "count" in rec["msg"], rec
            assert (got[0] == np.array([0, 0, 0, packed.VERDICT_WRITTEN | packed.VERDICT_REFILL], dtype=np.int32)).all(), got[0]
            assert not got[1].any() and not got[2].any() and not weights.any()
            # the next refill with a good count recovers
            rb.refill(_input(packed, b), count=_count_word(6))
            c = 6
            got = _outputs(rb.enqueue(bounds=BOUNDS, actions=actions), N)
            weights = rb.enqueue_weights().numpy()
        else:
            assert rec["flags"] == packed.REFILL_WRITTEN and rec["code"] == 0, rec
        mk = _mask([slice(0, c)])
        want = references("B", mk) if c else None
        _hold(packed, got, want, BOUNDS, mk, "count %d" % c, weights)
        if c:
            _clean_and_recovered(bpp, packed, got, want, b, mk, actions, BOUNDS, "count %d" % c)
    finally:
        rb.close()


# ---- 3. the live mask
MASKS = [("all live", ALL), ("all dead", _mask()), ("only slot 0", _mask([0])), ("only slot 69", _mask([69])),
         ("every other slot", _mask([slice(0, N, 2)])), ("group [5, 33) dead", _mask(dead=[slice(5, 33)])),
         ("every m = 4 slot dead", (MS != 4).astype(np.uint8)), ("bytes 2 and 255", _loud((np.random.default_rng(104).random(N) < 0.5).astype(np.uint8))),
         ("random", (np.random.default_rng(101).random(N) < 0.5).astype(np.uint8))]


def test_every_mask_equals_a_fresh_upload_of_the_live_rows(bpp, packed, corpora, references):
    params, a = corpora("A")
    _, b = corpora("B")
    actions = _actions(bpp)
    rb = packed.ResidentBatch.from_mixed(params, _input(packed, a))
    inputs = {"A": _input(packed, a), "B": _input(packed, b, pad=16, m_stride=6)}
    try:
        for i, (name, mk) in enumerate(MASKS + MASKS[::-1]):
            which = "B" if i % 2 == 0 else "A"
            d = b if which == "B" else a
            filled = rb.refill(inputs[which], live=_mask_dev(mk), shape_vectors=i % 3 != 0)
            got = _outputs(rb.enqueue(bounds=BOUNDS, actions=actions), N)
            weights = rb.enqueue_weights().numpy()
            rec = filled.result()
            assert rec["flags"] == packed.REFILL_WRITTEN and rec["code"] == 0, (name, rec)
            want = references(which, mk) if mk.any() else None
            _hold(packed, got, want, BOUNDS, mk, (name, which), weights)
            if mk.any():
                _clean_and_recovered(bpp, packed, got, want, d, mk, actions, BOUNDS, (name, which))
    finally:
        rb.close()


def test_t2_mask_rows(bpp, packed, corpora, references):
    """t = 2: two 32-byte rows per recovered mask, under a mask and under a count"""
    params, d = corpora("T2")
    RV = int(bpp.VerifyAction.RecoverAndVerify)
    inp = _input(packed, d)
    rb = packed.ResidentBatch.from_mixed(params, inp)
    try:
        for mk in (_mask([1, 3, 4, 8], n=N2), _mask(dead=[], n=N2), _mask([slice(0, 5)], n=N2)):
            if mk[:5].all() and not mk[5:].any():
                rb.refill(inp, count=_count_word(5), shape_vectors=False)
            else:
                rb.refill(inp, live=_mask_dev(mk))
            got = _outputs(rb.enqueue(actions=[RV]), N2, 2)
            want = references("T2", mk)
            _hold(packed, got, want, [0, N2], mk, "t = 2", rb.enqueue_weights().numpy())
            _clean_and_recovered(bpp, packed, got, want, d, mk, [RV], [0, N2], "t = 2")
            assert got[1].shape == (N2, 2, 32) and got[2].any()
    finally:
        rb.close()


# ---- 4. findings at the refill, at live and at dead slots
def _tamper(d, scalar_at=None, nonce_at=None, promise_at=None, foreign_at=None, flip_at=None):
    pr, sp, mv, mp = d["proofs"].copy(), d["seed_present"].copy(), d["min_values"].copy(), d["min_present"].copy()
    if scalar_at is not None:
        pr[scalar_at, D1:D1 + 32] = L_BYTES
    if nonce_at is not None:
        sp[nonce_at] = 1
    if promise_at is not None:
        mv[promise_at, 0], mp[promise_at, 0] = 1 << 32, 1
    if foreign_at is not None:
        pr[foreign_at, 0] = 2
    if flip_at is not None:
        pr[flip_at, R1] ^= 1
    return _with(d, proofs=pr, seed_present=sp, min_values=mv, min_present=mp)


def test_findings_at_the_refill(bpp, packed, corpora, references):
    params, a = corpora("A")
    _, b = corpora("B")
    actions = _actions(bpp)
    rb = packed.ResidentBatch.from_mixed(params, _input(packed, a))
    F = _mask(dead=[slice(6, 33, 3), 40, 47, 69])
    M4, M2, M1 = 35, 37, 36  # live slots of m = 4, m = 2 and m = 1
    assert MS[M4] == 4 and MS[M2] == 2 and MS[M1] == 1 and F[[M4, M2, M1, 5]].all() and MS[5] == 4
    DEAD4, DEAD2, DEAD1 = 40, 9, 15  # dead slots of m = 4, m = 2, m = 1
    assert MS[DEAD4] == 4 and MS[DEAD2] == 2 and MS[DEAD1] == 1 and not F[[DEAD4, DEAD2, DEAD1, 47]].any()
    live = _mask_dev(F)
    refill_flag = packed.VERDICT_WRITTEN | packed.VERDICT_REFILL

    def refused(d, mk):
        """what the fresh upload of the live rows throws"""
        with pytest.raises(bpp.ProofError) as err:
            packed.ResidentBatch.from_mixed(params, _input(packed, d, np.flatnonzero(mk))).close()
        return err.value

    try:
        # construction findings at live slots, each alone and two together (the lowest index wins), with and without a mask
        cases = [("a non-canonical scalar in an m = 4 proof", dict(scalar_at=M4), M4), ("a nonce on an m = 2 slot", dict(nonce_at=M2), M2),
                 ("two findings", dict(scalar_at=M2 + 5, nonce_at=M2), M2), ("two findings, the other order", dict(scalar_at=5, nonce_at=M2), 5)]
        for name, how, index in cases:
            d = _tamper(b, **how)
            for mk, kw in ((F, dict(live=live)), (ALL, dict())):
                filled = rb.refill(_input(packed, d), **kw)
                got = _outputs(rb.enqueue(bounds=BOUNDS, actions=actions), N)
                rec, err = filled.result(), refused(d, mk)
                assert rec["flags"] == packed.REFILL_WRITTEN | packed.REFILL_FINDING and rec["index"] == index and rec["tier"] == 1, (name, rec)
                assert rec["code"] == int(err.kind) and rec["msg"] == err.msg, (name, rec, err)
                want = np.array([rec["code"], 1, index, refill_flag], dtype=np.int32)
                assert (got[0] == want).all() and not got[1].any() and not got[2].any(), (name, got[0])
        # a foreign first byte: the fall-back, before a finding of lower index
        filled = rb.refill(_input(packed, _tamper(b, foreign_at=M1, scalar_at=5)), live=live)
        got = _outputs(rb.enqueue(bounds=BOUNDS, actions=actions), N)
        rec = filled.result()
        assert rec["flags"] == packed.REFILL_WRITTEN | packed.REFILL_FALLBACK and rec["code"] == 0 and rec["tier"] == 0, rec
        assert (got[0] == np.array([0, 0, 0, refill_flag], dtype=np.int32)).all() and not got[1].any() and not got[2].any(), got[0]
        # a good refill clears the flag
        assert rb.refill(_input(packed, b), live=live).result()["flags"] == packed.REFILL_WRITTEN
        got = _outputs(rb.enqueue(bounds=BOUNDS, actions=actions), N)
        _hold(packed, got, references("B", F), BOUNDS, F, "clean again", rb.enqueue_weights().numpy())
        # a promise above 2^32 and an invalid proof at live slots: the refill takes, the verification finds what it finds on the fresh upload
        for name, how, tier in (("a promise above the capacity", dict(promise_at=M4), 3), ("an invalid proof", dict(flip_at=M2), 7),
                                ("both, in one group", dict(promise_at=M1, flip_at=M4), 3)):
            d = _tamper(b, **how)
            assert rb.refill(_input(packed, d), live=live).result()["flags"] == packed.REFILL_WRITTEN, name
            got = _outputs(rb.enqueue(bounds=BOUNDS, actions=actions), N)
            want = _reference(packed, params, d, F, BOUNDS, actions, weights=False)
            assert want[0][2, 1] == tier, (name, want[0])
            _hold(packed, got, want, BOUNDS, F, name)
        # all of it at dead slots, with a count as well: no finding, no fall-back -- exactly the clean rows under the mask
        d = _tamper(b, scalar_at=DEAD4, nonce_at=DEAD2, promise_at=DEAD4, foreign_at=DEAD1, flip_at=47)
        assert rb.refill(_input(packed, d), live=live).result()["flags"] == packed.REFILL_WRITTEN
        got = _outputs(rb.enqueue(bounds=BOUNDS, actions=actions), N)
        _hold(packed, got, references("B", F), BOUNDS, F, "findings at dead slots", rb.enqueue_weights().numpy())
        assert (got[0][:, :3] == 0).all()
        d = _tamper(b, scalar_at=40, nonce_at=37, foreign_at=69, promise_at=35)
        assert rb.refill(_input(packed, d), count=_count_word(34)).result()["flags"] == packed.REFILL_WRITTEN
        mk = _mask([slice(0, 34)])
        _hold(packed, _outputs(rb.enqueue(bounds=BOUNDS, actions=actions), N), references("B", mk), BOUNDS, mk, "findings beyond the count")
    finally:
        rb.close()


# ---- 5. the early-out that follows from the shape: a slot whose proof does not fit its statement, dead or live
def test_a_dead_slot_of_unfitting_rounds_does_not_spare_the_live_proofs_the_final_check(bpp, packed, corpora):
    params, a = corpora("A")
    K = bpp.ProofErrorKind
    RV = int(bpp.VerifyAction.RecoverAndVerify)
    n, bad, flipped = 9, 3, 5
    # slot 3 (declared m = 1) holds the valid m = 2 proof of slot 2 and its first commitment; no nonce there
    d = {k: v[:n].copy() for k, v in a.items()}
    d["proofs"][bad], d["lens"][bad] = a["proofs"][2], a["lens"][2]
    d["commitments"][bad], d["min_values"][bad], d["min_present"][bad] = a["commitments"][2], 0, 0
    d["seed_present"][bad], d["seeds"][bad] = 0, 0
    rb = packed.ResidentBatch.from_mixed(params, _input(packed, d))
    try:
        res = packed.verify_groups(rb, [0, n])[0]
        assert res["code"] == int(K.InvalidLength) and res["index"] == bad and "Vector L/R length not adequate" in res["msg"], res
        tampered = _tamper(d, flip_at=flipped)
        ones, without = _mask(dead=[], n=n), _mask(dead=[bad], n=n)
        # the slot dead: one group over live proofs of which one is invalid -- the final check decides, as on the fresh upload
        rb.refill(_input(packed, tampered), live=_mask_dev(without))
        got = _outputs(rb.enqueue(actions=[RV]), n)
        want = _reference(packed, params, tampered, without, [0, n], [RV], weights=False)
        assert want[0][0, :2].tolist() == [int(K.VerificationFailed), 7] and want[0][0, 3] == packed.VERDICT_WRITTEN, want[0]
        _hold(packed, got, want, [0, n], without, "the slot dead")
        # ... with a count in front of the slot as well
        rb.refill(_input(packed, _tamper(d, flip_at=1)), count=_count_word(bad))
        got = _outputs(rb.enqueue(actions=[RV]), n)
        mk = _mask([slice(0, bad)], n=n)
        want = _reference(packed, params, _tamper(d, flip_at=1), mk, [0, n], [RV], weights=False)
        assert want[0][0, 1] == 7
        _hold(packed, got, want, [0, n], mk, "the slot beyond the count")
        # the slot live: its finding, whatever the other proofs are
        for kw in (dict(live=_mask_dev(ones)), dict()):
            rb.refill(_input(packed, tampered), **kw)
            got = _outputs(rb.enqueue(actions=[RV]), n)
            want = _reference(packed, params, tampered, ones, [0, n], [RV], weights=False)
            assert want[0].tolist() == [[int(K.InvalidLength), 6, bad, packed.VERDICT_WRITTEN]], want[0]  # the PASS-2 finding
            _hold(packed, got, want, [0, n], ones, "the slot live")
        # valid live proofs with the slot dead: Ok, and the masks of the nonce-bearing slots
        rb.refill(_input(packed, d), live=_mask_dev(without))
        got = _outputs(rb.enqueue(actions=[RV]), n)
        want = _reference(packed, params, d, without, [0, n], [RV])
        _hold(packed, got, want, [0, n], without, "valid and the slot dead", rb.enqueue_weights().numpy())
        _clean_and_recovered(bpp, packed, got, want, d, without, [RV], [0, n], "valid and the slot dead")
    finally:
        rb.close()


# ---- 6. refusals before any launch
def test_refusals_before_any_launch(bpp, packed, corpora):
    _, a = corpora("A")
    K = bpp.ProofErrorKind
    eng = bpp.Engine(0)
    params = bpp.RangeParameters.init(32, 4, bpp.create_pedersen_gens_with_extension_degree(1), engine=eng)
    inp = _input(packed, a)
    rb = packed.ResidentBatch.from_mixed(params, inp)
    lib = packed._lib
    keep = []

    def call(change=None, count=None, live=None, batch=None):
        st = lib.MixedBatch.from_buffer_copy(inp.struct)
        st.transcript_state, st.transcript_label, st.label_len = None, None, 0
        if change:
            change(st)
        rc = eng.lib.bpp_batch_refill_enqueue_mixed(eng.ctx, (batch or rb).handle, ctypes.byref(st), count, live, None, None)
        return rc, eng.lib.bpp_ctx_last_error(eng.ctx).decode()

    def vectors(lens=None, m=None):
        """the batch's vectors with entries replaced"""
        ln, mm = a["lens"].copy(), a["m"].copy()
        for i, v in (lens or {}).items():
            ln[i] = v
        for i, v in (m or {}).items():
            mm[i] = v
        keep.extend([ln, mm])

        def change(st):
            st.proof_lens, st.m = ln.ctypes.data, mm.ctypes.data
        return change

    def setf(**fields):
        def change(st):
            for k, v in fields.items():
                setattr(st, k, v)
        return change

    try:
        before = (packed.refill_stats(eng), packed.enqueue_stats(eng))
        longest, word, mask_dev = int(a["lens"].max()), _count_word(5), _mask_dev(ALL)
        lens_dev = torch.from_numpy(a["lens"].astype(np.int64)).cuda()
        host_mask, label = np.ones(N, dtype=np.uint8), np.frombuffer(LABEL, dtype=np.uint8).copy()
        refusals = [
            ("proof_lens[17]", vectors(lens={17: int(a["lens"][17]) + 64})), ("proof_lens[0]", vectors(lens={0: int(a["lens"][0]) - 64, 30: 1})),
            ("m[69]", vectors(m={69: 1})), ("m[4]", vectors(m={4: 4, 9: 1})), ("proof_lens[3]", vectors(lens={3: 1}, m={3: 2, 5: 2})),
            ("n_items", setf(n_items=N - 1)), ("n_items", setf(n_items=N + 1)),
            ("seed_nonces32", setf(seed_nonces32=None, seed_present=None)), ("seed_present", setf(seed_present=None)),
            ("min_values", setf(min_values=None, min_present=None)), ("min_present", setf(min_present=None)),
            ("give both", setf(proof_lens=None)), ("give both", setf(m=None)),
            ("proof_lens is device memory", setf(proof_lens=lens_dev.data_ptr())),
            ("proof_stride is below", setf(proof_stride=longest - 1)), ("m_stride is below", setf(m_stride=3)),
            ("transcript", setf(transcript_label=label.ctypes.data, label_len=len(LABEL))), ("transcript", setf(transcript_state=label.ctypes.data)),
            ("proofs / commitments32: null", setf(proofs=None)), ("commitments32: not device memory", setf(commitments32=a["commitments"].ctypes.data)),
        ]
        for text, change in refusals:
            rc, msg = call(change)
            assert rc == int(K.InvalidArgument) and text in msg, (text, rc, msg)
        rc, msg = call(count=ctypes.c_void_p(word.data_ptr()), live=ctypes.c_void_p(mask_dev.data_ptr()))
        assert rc == int(K.InvalidArgument) and "count_dev and live_dev" in msg, msg
        rc, msg = call(live=ctypes.c_void_p(host_mask.ctypes.data))
        assert rc == int(K.InvalidArgument) and "live_dev: not device memory" in msg, msg
        rc, msg = call(count=ctypes.c_void_p(word.data_ptr() + 2))
        assert rc == int(K.InvalidArgument) and "count_dev" in msg, msg
        # batches of other origins: the packed device upload, the host mixed form
        first = np.flatnonzero(MS == 1)[:4]
        pk = packed.DevicePackedInput(_dev(a["proofs"][first][:, :int(a["lens"][first[0]])]), _dev(a["commitments"][first][:, :1]),
                                      _dev(a["min_values"][first][:, :1]), _dev(a["min_present"][first][:, :1]), _dev(a["seeds"][first]), LABEL)
        torch.cuda.synchronize()
        packed_rb = packed.ResidentBatch(params, pk, None, None, None, None, LABEL, form="device")
        host_rb = packed.ResidentBatch.from_mixed(params, packed.MixedInput(a["proofs"], a["lens"], a["m"], a["commitments"], a["min_values"],
                                                                            a["min_present"], a["seeds"], LABEL, seed_present=a["seed_present"]))
        for other in (packed_rb, host_rb):
            rc, msg = call(batch=other)
            assert rc == int(K.InvalidArgument) and "bpp_batch_upload_mixed_device packed on the device" in msg, msg
        with pytest.raises(bpp.ProofError) as e:
            packed_rb.refill(inp)  # (a DeviceMixedInput reaches the mixed call)
        assert "bpp_batch_upload_mixed_device" in e.value.msg
        # the packed calls on a mixed batch: today's text, through the dispatch on the input's type
        with pytest.raises(bpp.ProofError) as e:
            rb.refill(pk)
        assert e.value.kind == K.InvalidArgument and "only a batch that bpp_batch_upload_packed_device packed on the device records its shape" in e.value.msg
        with pytest.raises(bpp.ProofError):
            rb.refill(inp, count=5, live=mask_dev)  # (the binding's own refusal)
        assert (packed.refill_stats(eng), packed.enqueue_stats(eng)) == before
        rb.verify_only()  # nothing was launched: the batch is still the host's
        packed_rb.close()
        host_rb.close()
    finally:
        torch.cuda.synchronize()
        rb.close()
        params.close()
        eng.close()


# ---- 7. the steady state and the secrets
def test_steady_state_and_secrets(bpp, packed, corpora, references):
    _, a = corpora("A")
    _, b = corpora("B")
    actions = _actions(bpp)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        eng = bpp.Engine(0, stream=stream.cuda_stream)
        params = bpp.RangeParameters.init(32, 4, bpp.create_pedersen_gens_with_extension_degree(1), engine=eng)
        inputs = {"A": _input(packed, a), "B": _input(packed, b, pad=8)}
        rb = packed.ResidentBatch.from_mixed(params, inputs["A"])
        masks = [m for _, m in MASKS if m.any()]
        dev_masks = [_mask_dev(m) for m in masks]
        try:
            r0 = packed.refill_stats(eng)
            rb.refill(inputs["B"], shape_vectors=False).result()  # the first refill: the batch's words
            rb.enqueue(bounds=BOUNDS, actions=actions).wait()  # (the layout is planned here, with nothing in flight)
            r1, e1 = packed.refill_stats(eng), packed.enqueue_stats(eng)
            assert r1["first_calls"] == r0["first_calls"] + 1
            runs = []
            for step in range(8):
                which = "AB"[step % 2]
                k = step % len(masks)
                rb.refill(inputs[which], live=dev_masks[k], shape_vectors=False)
                runs.append((which, masks[k], rb.enqueue(bounds=BOUNDS, actions=actions), rb.enqueue_weights()))
            r2, e2 = packed.refill_stats(eng), packed.enqueue_stats(eng)  # (before any wait)
            assert r2["host_waits"] == 0 and e2["host_waits"] == e1["host_waits"] == 0
            assert r2["calls"] == r1["calls"] + 8 and e2["calls"] == e1["calls"] + 8
            assert e2["layouts_in_call"] == e1["layouts_in_call"]
            assert r2["first_calls"] == r1["first_calls"] + 1  # the first mask, and nothing after it
            for which, mk, e, w in runs:
                _hold(packed, _outputs(e, N), references(which, mk), BOUNDS, mk, ("steady", which), w.numpy())
            # secrets: the nonces of the live nonce-bearing slots, and none once no such slot is live
            some = _mask([slice(0, 40)])
            rb.refill(inputs["A"], live=_mask_dev(some))
            assert _secret_bytes(eng, rb.handle) == np.count_nonzero(a["seeds"][(some != 0) & (a["seed_present"] != 0)]) > 0
            rb.refill(inputs["B"], live=_mask_dev((MS != 1).astype(np.uint8)))
            assert _secret_bytes(eng, rb.handle) == 0
        finally:
            torch.cuda.synchronize()
            rb.close()
            params.close()
            eng.close()
