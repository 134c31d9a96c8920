"""GPU tests: a resident batch is refilled under a per-item live mask (bpp_batch_refill_enqueue_live, csrc/refill.h,
csrc/chain_dev.h, csrc/verdict.h), the mask being N bytes in device memory that are read on the stream.

The reference in every comparison is a FRESH bpp_batch_upload_packed_device of the LIVE ITEMS ALONE, in slot order, with the group
boundaries mapped to the compacted arrays and empty groups dropped: its enqueued records, masks and mask_present, and -- for the
weights, which verdicts cannot pin: any non-zero weights accept a valid proof -- BPP_TRACE_WEIGHTS of a blocking call on that fresh
upload, which runs the host chain, scattered back to the slots.  A record's `index` is mapped from the reference's k-th live item of
the group to that item's slot offset.  A refilled batch is never compared against its own output.  References are made once per
(corpus, mask) and shared.

Boundaries [0, 5, 70, 200, 320]: the masks put holes inside groups, whole groups dead between live ones, a whole 64-slot window of the
chain without a live lane, one below / at / one above the chain's 64-proof stage of live slots with gaps, and live slots on both
sides of the verdict scan's 256-proof workgroup."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from tests.helpers import LABEL

pytestmark = pytest.mark.gpu

L_BYTES = np.frombuffer(bytes.fromhex("edd3f55c1a631258d69cf7a2def9de14" + "00" * 15 + "10"), dtype=np.uint8)  # the group order
R1 = 1 + 32 + 96  # t = 1: [t] d1 A A1 B r1 s1 (L R)*
S1 = R1 + 32
A_POINT = 1 + 32  # the member A
N, BOUNDS = 320, [0, 5, 70, 200, 320]
N2, CHUNK2 = 24, 8


def _mask(live=(), dead=None, n=N):
    """ones at `live` (an iterable of slots or slices); with `dead`: ones everywhere but there"""
    mk = np.zeros(n, dtype=np.uint8) if dead is None else np.ones(n, dtype=np.uint8)
    for s in (live if dead is None else dead):
        mk[s] = 0 if dead is not None else 1
    return mk


def _random(seed, n=N, density=0.5):
    return (np.random.default_rng(seed).random(n) < density).astype(np.uint8)


def _gaps(k):
    """exactly k live slots inside [70, 200), every other slot from 71 on; the other groups fully live"""
    mk = _mask(dead=[slice(70, 200)])
    mk[71:71 + 2 * k:2] = 1
    assert mk[70:200].sum() == k
    return mk


def _loud(mk):
    """the same mask with 2 and 255 for "live" """
    out = mk.copy()
    idx = np.flatnonzero(mk)
    out[idx[::2]] = 2
    out[idx[1::2]] = 255
    return out


PREFIXES = [5, 6, 134]
MASKS = ([("all live", _mask(dead=[])), ("all dead", _mask())] +
         [("prefix %d" % c, _mask([slice(0, c)])) for c in PREFIXES] +
         [("only slot %d" % s, _mask([s])) for s in (0, 4, 5, 69, 319)] +
         [("every other slot", _mask([slice(0, N, 2)])),
          ("group [5, 70) dead", _mask(dead=[slice(5, 70)])),
          ("slots 70..133 dead", _mask(dead=[slice(70, 134)])),
          ("63 live with gaps", _gaps(63)), ("64 live with gaps", _gaps(64)), ("65 live with gaps", _gaps(65)),
          ("slots 255, 256, 257", _mask([255, 256, 257])),
          ("random 1", _random(101)), ("random 2", _random(102)), ("random 3", _random(103)),
          ("bytes 2 and 255", _loud(_random(104)))])
assert MASKS[10][1][70:200].sum() == 65  # every other slot: 65 live in [70, 200), across the chain's 64-proof stage
MASKS2 = [("none", _mask(n=N2)), ("slot 7 only", _mask([7], n=N2)), ("8..15 dead", _mask(dead=[slice(8, 16)], n=N2)),
          ("alternating", _mask([slice(0, N2, 2)], n=N2)), ("all", _mask(dead=[], n=N2))]
# the mask of the findings, secrets and form tests: holes in every group but the first, a whole dead run across a 64-slot window
F = _mask(dead=[slice(5, 70, 2), slice(71, 200, 3), slice(230, 300)])


@pytest.fixture(scope="module")
def packed():
    return importlib.import_module("bulletproofs-plus_amd.packed")


@pytest.fixture(scope="module")
def corpora(bpp, packed, engine):
    """m -> (params, arrays): 320 valid proofs with seed nonces at m = 1, 24 at m = 2; made once, read-only"""
    import bench
    made = {}

    def get(m):
        if m not in made:
            params = bpp.RangeParameters.init(32, m, bpp.create_pedersen_gens_with_extension_degree(1), engine=engine)
            d = bench.make_inputs(np, packed, params, N if m == 1 else N2, seed=9500 + m)
            if d["seeds"] is None:  # (m = 2: a nonce array that no item uses still shapes the batch)
                d["seeds"] = np.random.default_rng(m).integers(1, 256, size=(d["proofs"].shape[0], 32), dtype=np.uint8)
            for a in d.values():
                a.setflags(write=False)
            made[m] = (params, d)
        return made[m]

    yield get
    for params, _ in made.values():
        params.close()


def _dev(a):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:
        a = a.copy()
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).cuda()


def _input(packed, d, slots, m=1, proofs=None, seed_present=None):
    """the items at `slots` (an index array or a slice), in that order, as a DevicePackedInput (nonces on every item at m = 1, on none
    at m = 2)"""
    pr = (d["proofs"] if proofs is None else proofs)[slots]
    if seed_present is None and m != 1:
        seed_present = np.zeros(len(pr), dtype=np.uint8)
    elif seed_present is not None:
        seed_present = seed_present[slots]
    inp = packed.DevicePackedInput(_dev(pr), _dev(d["commitments"][slots]), _dev(d["min_values"][slots]), _dev(d["min_present"][slots]),
                                   _dev(d["seeds"][slots]), LABEL, seed_present=_dev(seed_present))
    torch.cuda.synchronize()
    return inp


def _actions(bpp):
    V, RV, RO = (int(bpp.VerifyAction.VerifyOnly), int(bpp.VerifyAction.RecoverAndVerify), int(bpp.VerifyAction.RecoverOnly))
    return [RV, V, RV, RO]


def _chunks(n, chunk):
    return list(range(0, n, chunk)) + [n]


def _outputs(e, n=None):
    """(verdicts, masks, present) on the host; a call in which no group recovers hands out no masks: zeros for `n` items"""
    e.wait()
    if e.masks is None:
        return (e.verdicts.cpu().numpy().copy(), np.zeros((n, 1, 32), dtype=np.uint8), np.zeros(n, dtype=np.uint8))
    return (e.verdicts.cpu().numpy().copy(), e.masks.cpu().numpy().copy(), e.present.cpu().numpy().copy())


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


def _reference(packed, params, d, mk, bounds, actions, m=1, proofs=None, weights=True):
    """a fresh upload of the live items alone, the boundaries mapped and empty groups dropped: (verdicts, masks, present, weights of a
    blocking call), the last three in compacted order"""
    groups = _groups(bounds, mk)
    slots = np.flatnonzero(mk)
    cb, acts = [0], []
    for g, s in enumerate(groups):
        if len(s):
            cb.append(cb[-1] + len(s))
            acts.append(actions[g])
    rb = packed.ResidentBatch(params, _input(packed, d, slots, m, proofs=proofs), None, None, None, None, LABEL, form="device")
    try:
        out = _outputs(rb.enqueue(bounds=cb, actions=acts), len(slots))
        w = None
        if weights:
            packed.verify_groups(rb, cb)
            w = np.frombuffer(rb.trace(3), dtype=np.uint8).reshape(len(slots), 32).copy()
        return out + (w,)
    finally:
        rb.close()


@pytest.fixture(scope="module")
def references(bpp, packed, corpora):
    """(m, mask) -> the reference of the clean corpus under the mask, made on first use and never changed"""
    made = {}

    def get(m, mk):
        key = (m, (mk != 0).tobytes())
        if key not in made:
            params, d = corpora(m)
            if m == 1:
                made[key] = _reference(packed, params, d, mk, BOUNDS, _actions(bpp))
            else:
                RV, RO = int(bpp.VerifyAction.RecoverAndVerify), int(bpp.VerifyAction.RecoverOnly)
                made[key] = _reference(packed, params, d, mk, _chunks(N2, CHUNK2), [RO, RV, RO], m=2)
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


def _secret_bytes(eng, handle=0):
    k = ctypes.c_uint64()
    assert eng.lib.bpp_batch_secret_bytes(eng.ctx, handle, ctypes.byref(k)) == 0
    return k.value


# ---- 1. one batch, every mask, in sequence and shuffled; records, masks and weights
def test_every_mask_equals_a_fresh_upload_of_the_live_items(bpp, packed, engine, corpora, references):
    params, d = corpora(1)
    actions = _actions(bpp)
    inp = _input(packed, d, slice(0, N))
    rb = packed.ResidentBatch(params, inp, None, None, None, None, LABEL, form="device")
    order = list(range(len(MASKS))) + [int(k) for k in np.random.default_rng(7).permutation(len(MASKS))]
    try:
        for i in order:
            name, mk = MASKS[i]
            filled = rb.refill(inp, live=_mask_dev(mk))
            got = _outputs(rb.enqueue(bounds=BOUNDS, actions=actions))
            weights = rb.enqueue_weights().numpy()
            rec = filled.result()
            assert rec["flags"] == packed.REFILL_WRITTEN and rec["code"] == 0, (name, rec)
            want = references(1, mk) if mk.any() else None
            _hold(packed, got, want, BOUNDS, mk, name, weights)
            if mk.any():  # valid proofs: every live group is Ok, and the masks are the openings' blinding factors where the group recovers
                assert (want[0][:, :3] == 0).all() and (want[0][:, 3] == packed.VERDICT_WRITTEN).all(), want[0]
                recovers = np.zeros(N, dtype=bool)
                for g in range(len(BOUNDS) - 1):
                    if actions[g] != int(bpp.VerifyAction.VerifyOnly):
                        recovers[BOUNDS[g]:BOUNDS[g + 1]] = True
                recovers &= mk != 0
                assert got[2].tolist() == recovers.astype(np.uint8).tolist(), name
                assert got[1][recovers].tobytes() == d["blindings"][:, 0][recovers].tobytes(), name
            if name.startswith("prefix "):  # ... and, byte for byte, what a count refill with that c gives on the same batch
                c = int(name.split()[1])
                rb.refill(inp, count=_count_word(c))
                again = _outputs(rb.enqueue(bounds=BOUNDS, actions=actions))
                for x, y in zip(got, again):
                    assert x.tobytes() == y.tobytes(), name
                assert rb.enqueue_weights().numpy().tobytes() == weights.tobytes(), name
    finally:
        rb.close()


# ---- 2. findings at live and at dead slots
def test_findings_at_live_slots_are_reported_and_at_dead_slots_have_no_effect(bpp, packed, engine, corpora, references):
    params, d = corpora(1)
    actions = _actions(bpp)
    clean = _input(packed, d, slice(0, N))
    rb = packed.ResidentBatch(params, clean, None, None, None, None, LABEL, form="device")
    live = _mask_dev(F)
    assert F[[20, 100, 133, 90, 8]].all() and not F[[9, 74, 250, 299, 11, 7]].any()

    def tampered(at):
        """the four findings at four indices: [invalid, identity member, non-canonical scalar, foreign first byte]"""
        pr = d["proofs"].copy()
        i = at[0]
        if i is not None:
            pr[i, R1] ^= 1
        i = at[1]
        if i is not None:
            pr[i, A_POINT:A_POINT + 32] = 0
        i = at[2]
        if i is not None:
            pr[i, S1:S1 + 32] = L_BYTES
        i = at[3]
        if i is not None:
            pr[i, 0] = 2
        return pr

    try:
        # at dead slots, all four at once, and a missing nonce there: exactly the clean batch under the mask
        pr = tampered([9, 74, 250, 299])
        sp = np.ones(N, dtype=np.uint8)
        sp[11] = 0
        filled = rb.refill(_input(packed, d, slice(0, N), proofs=pr, seed_present=sp), live=live)
        got = _outputs(rb.enqueue(bounds=BOUNDS, actions=actions))
        rec = filled.result()
        assert rec["flags"] == packed.REFILL_WRITTEN and rec["code"] == 0 and rec["msg"] == "", rec
        _hold(packed, got, references(1, F), BOUNDS, F, "findings at dead slots")
        assert (got[0][:, :3] == 0).all()
        # at live slots, what verification finds: the fresh upload's records with the index as a slot offset (slot 20 is the 8th live
        # item of group [5, 70): the reference says 7, the refilled batch 15)
        for name, at, tier in (("invalid proof", [100, None, None, None], 7), ("identity member", [None, 20, None, None], 5),
                               ("both, in two groups", [133, 20, None, None], 7)):
            pr = tampered(at)
            filled = rb.refill(_input(packed, d, slice(0, N), proofs=pr), live=live)
            got = _outputs(rb.enqueue(bounds=BOUNDS, actions=actions))
            assert filled.result()["flags"] == packed.REFILL_WRITTEN, name
            want = _reference(packed, params, d, F, BOUNDS, actions, proofs=pr, weights=False)
            assert tier in want[0][:, 1].tolist(), (name, want[0])
            _hold(packed, got, want, BOUNDS, F, name)
            if at[1] is not None:
                assert want[0][1, 1:].tolist() == [5, 7, packed.VERDICT_WRITTEN], want[0]
                assert got[0][1, 2] == 15
        # at a live slot, what the upload refuses: its code and text, the SLOT in the record; nothing of the verification is claimed
        pr = tampered([None, None, 90, None])
        pr[74, S1:S1 + 32] = L_BYTES  # (a second one at a dead slot in front of it changes nothing)
        filled = rb.refill(_input(packed, d, slice(0, N), proofs=pr), live=live)
        got = _outputs(rb.enqueue(bounds=BOUNDS, actions=actions))
        rec = filled.result()
        with pytest.raises(bpp.ProofError) as err:
            packed.ResidentBatch(params, _input(packed, d, np.flatnonzero(F), proofs=pr), None, None, None, None, LABEL, form="device")
        assert rec["flags"] == packed.REFILL_WRITTEN | packed.REFILL_FINDING and rec["index"] == 90, rec
        assert rec["code"] == int(err.value.kind) and rec["msg"] == err.value.msg, (rec, err.value)
        want = np.array([rec["code"], 1, 90, packed.VERDICT_WRITTEN | packed.VERDICT_REFILL], dtype=np.int32)
        assert (got[0] == want).all() and not got[1].any() and not got[2].any(), got[0]
        # a foreign first byte: the fall-back at a live slot, nothing at a dead one
        filled = rb.refill(_input(packed, d, slice(0, N), proofs=tampered([None, None, None, 8])), live=live)
        got = _outputs(rb.enqueue(bounds=BOUNDS, actions=actions))
        rec = filled.result()
        assert rec["flags"] == packed.REFILL_WRITTEN | packed.REFILL_FALLBACK and rec["code"] == 0, rec
        assert (got[0] == np.array([0, 0, 0, packed.VERDICT_WRITTEN | packed.VERDICT_REFILL], dtype=np.int32)).all(), got[0]
        filled = rb.refill(_input(packed, d, slice(0, N), proofs=tampered([None, None, None, 7])), live=live)
        got = _outputs(rb.enqueue(bounds=BOUNDS, actions=actions))
        assert filled.result()["flags"] == packed.REFILL_WRITTEN
        _hold(packed, got, references(1, F), BOUNDS, F, "a foreign first byte at a dead slot")
        # ... and the batch recovers
        rb.refill(clean, live=live)
        _hold(packed, _outputs(rb.enqueue(bounds=BOUNDS, actions=actions)), references(1, F), BOUNDS, F, "clean again")
    finally:
        rb.close()


# ---- 3. a zero weight: only a live item's raises the redraw
def test_a_zero_weight_redraws_for_live_items_only(bpp, packed, corpora, references):
    _, d = corpora(1)
    actions = _actions(bpp)
    eng = bpp.Engine(0)
    params = bpp.RangeParameters.init(32, 1, bpp.create_pedersen_gens_with_extension_degree(1), engine=eng)
    inp = _input(packed, d, slice(0, N))
    rb = packed.ResidentBatch(params, inp, None, None, None, None, LABEL, form="device")
    mk = _mask(dead=[slice(5, 70), slice(71, 200, 3)])  # group 1 is empty
    try:
        rb.refill(inp, live=_mask_dev(mk))
        want = references(1, mk)
        eng.set_option("chain_test_zero", 10 + 1)  # a dead slot of the empty group, then one inside a live group
        _hold(packed, _outputs(rb.enqueue(bounds=BOUNDS, actions=actions)), want, BOUNDS, mk, "a forced zero at slot 10")
        eng.set_option("chain_test_zero", 74 + 1)
        _hold(packed, _outputs(rb.enqueue(bounds=BOUNDS, actions=actions)), want, BOUNDS, mk, "a forced zero at slot 74")
        eng.set_option("chain_test_zero", 72 + 1)  # a live slot: the groups that hold live items and are held to the final check
        got = _outputs(rb.enqueue(bounds=BOUNDS, actions=actions))
        redraw = [0, 0, 0, packed.VERDICT_WRITTEN | packed.VERDICT_REDRAW]
        assert got[0][0].tolist() == redraw and got[0][2].tolist() == redraw, got[0]
        assert (got[0][1] == _empty_record(packed)).all(), got[0]
        assert got[0][3].tolist() == want[0][2].tolist()  # (RecoverOnly: never held to the final check)
        eng.set_option("chain_test_zero", 0)
        _hold(packed, _outputs(rb.enqueue(bounds=BOUNDS, actions=actions)), want, BOUNDS, mk, "no forced zero")
    finally:
        eng.set_option("chain_test_zero", 0)
        torch.cuda.synchronize()
        rb.close()
        params.close()
        eng.close()


# ---- 4. secrets, form switches, refusals
def test_secrets_form_switches_and_refusals(bpp, packed, corpora, references):
    _, d = corpora(1)
    actions = _actions(bpp)
    eng = bpp.Engine(0)
    params = bpp.RangeParameters.init(32, 1, bpp.create_pedersen_gens_with_extension_degree(1), engine=eng)
    inp = _input(packed, d, slice(0, N))
    rb = packed.ResidentBatch(params, inp, None, None, None, None, LABEL, form="device")
    K = bpp.ProofErrorKind
    try:
        # a mask in host memory: refused with the field named, nothing launched
        host = np.ones(N, dtype=np.uint8)
        st = packed._lib.PackedBatch.from_buffer_copy(inp.struct)
        st.transcript_label, st.transcript_state, st.label_len = None, None, 0
        before = (packed.refill_stats(eng), packed.enqueue_stats(eng))
        rc = eng.lib.bpp_batch_refill_enqueue_live(eng.ctx, rb.handle, ctypes.byref(st), ctypes.c_void_p(host.ctypes.data), None, None)
        assert rc == int(K.InvalidArgument) and b"live_dev" in eng.lib.bpp_ctx_last_error(eng.ctx)
        assert (packed.refill_stats(eng), packed.enqueue_stats(eng)) == before
        rb.verify_only()  # (and the batch is still the host's)
        # a mask and a count: raised before any call
        with pytest.raises(bpp.ProofError) as e:
            rb.refill(inp, count=5, live=_mask_dev(F))
        assert e.value.kind == K.InvalidArgument and (packed.refill_stats(eng), packed.enqueue_stats(eng)) == before
        with pytest.raises(bpp.ProofError):
            rb.refill(inp, live=_mask_dev(F[:-1]))
        assert packed.refill_stats(eng) == before[0]
        # mask -> count -> plain -> mask: the batch is in the form of its last refill; the secrets are the live items' nonces
        ones = _mask(dead=[])
        assert np.count_nonzero(d["seeds"][F == 0]) > 0
        for form, mk in (("mask", F), ("count", _mask([slice(0, 134)])), ("plain", ones), ("mask", MASKS[10][1]), ("count", _mask([slice(0, 6)])),
                         ("mask", F), ("plain", ones)):
            if form == "mask":
                rb.refill(inp, live=_mask_dev(mk))
            elif form == "count":
                rb.refill(inp, count=_count_word(int(mk.sum())))
            else:
                rb.refill(inp)
            assert _secret_bytes(eng, rb.handle) == np.count_nonzero(d["seeds"][mk != 0]), form
            got = _outputs(rb.enqueue(bounds=BOUNDS, actions=actions))
            _hold(packed, got, references(1, mk), BOUNDS, mk, form, rb.enqueue_weights().numpy())
        # a null mask is the plain refill, through the new entry point
        rb.refill(inp, live=_mask_dev(F))
        assert eng.lib.bpp_batch_refill_enqueue_live(eng.ctx, rb.handle, ctypes.byref(st), None, None, None) == 0
        _hold(packed, _outputs(rb.enqueue(bounds=BOUNDS, actions=actions)), references(1, ones), BOUNDS, ones, "null mask", rb.enqueue_weights().numpy())
        # an empty group's text, and one group over the whole batch (the one-group MSM plan) under a mask and under none
        rb.refill(inp, live=_mask_dev(_mask(dead=[slice(5, 70)])))
        res = rb.enqueue(bounds=BOUNDS, actions=actions).results()
        assert res[1]["code"] == 0 and res[1]["tier"] == 0 and "no live item" in res[1]["msg"] and res[0]["msg"] == ""
        RV = bpp.VerifyAction.RecoverAndVerify
        only = _mask([255, 256, 257])
        rb.refill(inp, live=_mask_dev(only))
        got = _outputs(rb.enqueue(action=RV))
        assert got[0].tolist() == [[0, 0, 0, packed.VERDICT_WRITTEN]] and got[2].tolist() == only.tolist()
        assert got[1][only != 0].tobytes() == d["blindings"][:, 0][only != 0].tobytes() and not got[1][only == 0].any()
        rb.refill(inp, live=_mask_dev(_mask()))
        got = _outputs(rb.enqueue(action=RV))
        assert (got[0] == _empty_record(packed)).all() and not got[1].any() and not got[2].any()
        assert _secret_bytes(eng, rb.handle) == 0
    finally:
        torch.cuda.synchronize()
        rb.close()
        params.close()
        eng.close()


# ---- 5. the mask is read on the stream, and only by the refill
def test_the_mask_is_read_in_stream_order(bpp, packed, corpora, references):
    _, d = corpora(1)
    actions = _actions(bpp)
    A, B = F, MASKS[10][1]
    want_a, want_b = references(1, A), references(1, B)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        eng = bpp.Engine(0, stream=stream.cuda_stream)
        params = bpp.RangeParameters.init(32, 1, bpp.create_pedersen_gens_with_extension_degree(1), engine=eng)
        inp = packed.DevicePackedInput(_dev(d["proofs"]), _dev(d["commitments"]), _dev(d["min_values"]), _dev(d["min_present"]), _dev(d["seeds"]), LABEL)
        rb = packed.ResidentBatch(params, inp, None, None, None, None, LABEL, form="device")
        mask = torch.ones((N,), dtype=torch.uint8, device="cuda")
        dev_a, dev_b = torch.from_numpy(A.copy()).cuda(), torch.from_numpy(_loud(B)).cuda()
        staged = torch.from_numpy(np.stack([A, np.zeros(N, dtype=np.uint8)])).pin_memory()
        rb.refill(inp, live=mask).result()
        rb.enqueue(bounds=BOUNDS, actions=actions).wait()  # (the layout is planned here, with nothing in flight)
        r0, e0 = packed.refill_stats(eng), packed.enqueue_stats(eng)
        # from here on nothing waits: the mask is written by a kernel just before the refill and overwritten just after it
        mask.copy_(dev_a)
        rb.refill(inp, live=mask)
        mask.fill_(0)
        first = rb.enqueue(bounds=BOUNDS, actions=actions)
        w_first = rb.enqueue_weights()
        mask.fill_(1)
        second = rb.enqueue(bounds=BOUNDS, actions=actions)  # a later enqueue reads the batch's own copy
        # ... with other byte values for "live"
        mask.copy_(dev_b)
        rb.refill(inp, live=mask)
        mask.fill_(0)
        third = rb.enqueue(bounds=BOUNDS, actions=actions)
        # ... and by an asynchronous copy
        mask.copy_(staged[0], non_blocking=True)
        rb.refill(inp, live=mask)
        mask.copy_(staged[1], non_blocking=True)
        fourth = rb.enqueue(bounds=BOUNDS, actions=actions)
        r1, e1 = packed.refill_stats(eng), packed.enqueue_stats(eng)  # (before any wait)
        assert r1["host_waits"] == 0 and r1["calls"] == r0["calls"] + 3 and r1["first_calls"] == 1
        assert e1["host_waits"] == e0["host_waits"] == 0 and e1["layouts_in_call"] == e0["layouts_in_call"] and e1["calls"] == e0["calls"] + 4
        _hold(packed, _outputs(first), want_a, BOUNDS, A, "written before the refill", w_first.numpy())
        _hold(packed, _outputs(second), want_a, BOUNDS, A, "overwritten after the refill")
        _hold(packed, _outputs(third), want_b, BOUNDS, B, "bytes 2 and 255")
        _hold(packed, _outputs(fourth), want_a, BOUNDS, A, "an asynchronous copy")
        assert not mask.cpu().numpy().any()
        rb.close()
        params.close()
        eng.close()


# ---- 6. aggregated proofs, equal chunks, actions per group
@pytest.mark.parametrize("which", range(len(MASKS2)), ids=[name.replace(" ", "_") for name, _ in MASKS2])
def test_m2_chunks_with_actions(bpp, packed, engine, corpora, references, which):
    params, d = corpora(2)
    name, mk = MASKS2[which]
    RV, RO = int(bpp.VerifyAction.RecoverAndVerify), int(bpp.VerifyAction.RecoverOnly)
    inp = _input(packed, d, slice(0, N2), m=2)
    rb = packed.ResidentBatch(params, inp, None, None, None, None, LABEL, form="device")
    try:
        filled = rb.refill(inp, live=_mask_dev(mk))
        got = _outputs(rb.enqueue(chunk=CHUNK2, actions=[RO, RV, RO]))
        weights = rb.enqueue_weights().numpy()
        assert filled.result()["flags"] == packed.REFILL_WRITTEN
        want = references(2, mk) if mk.any() else None
        _hold(packed, got, want, _chunks(N2, CHUNK2), mk, name, weights)
        if mk.any():
            assert (want[0][:, :3] == 0).all()
    finally:
        rb.close()
