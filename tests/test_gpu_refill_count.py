"""GPU tests: a resident batch is refilled with fewer items than it holds (bpp_batch_refill_enqueue_count, csrc/refill.h,
csrc/chain_dev.h, csrc/verdict.h), the count being one word in device memory that is read on the stream.

The reference in every comparison is a FRESH bpp_batch_upload_packed_device of the FIRST c ITEMS of the same arrays with the group
boundaries clipped to c: its enqueued records, masks and mask_present, and -- for the weights, which verdicts cannot pin: any non-zero
weights accept a valid proof -- BPP_TRACE_WEIGHTS of a blocking call on that fresh upload, which runs the host chain.  A refilled batch
is never compared against its own output.  References are made once per (corpus, count) and shared.

Boundaries [0, 5, 70, 200, 320] and the counts below put the cut inside the first group, on a boundary, one either side of one, one
below / at / one above a multiple of the chain's 64-proof stage inside a group (70 + 64 = 134), across the verdict scan's 256-proof
workgroup, and at the full batch."""
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
COUNTS = [0, 1, 5, 6, 69, 70, 133, 134, 135, 199, 200, 257, 319, 320]
N2, CHUNK2, COUNTS2 = 24, 8, [0, 7, 8, 9, 24]


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


def _input(packed, d, n, m=1, proofs=None, seed_present=None):
    """the first n items as a DevicePackedInput (nonces on every item at m = 1, on none at m = 2)"""
    if seed_present is None and m != 1:
        seed_present = np.zeros(n, dtype=np.uint8)
    inp = packed.DevicePackedInput(_dev((d["proofs"] if proofs is None else proofs)[:n]), _dev(d["commitments"][:n]), _dev(d["min_values"][:n]),
                                   _dev(d["min_present"][:n]), _dev(d["seeds"][:n]), LABEL, seed_present=_dev(seed_present))
    torch.cuda.synchronize()
    return inp


def _actions(bpp):
    V, RV, RO = (int(bpp.VerifyAction.VerifyOnly), int(bpp.VerifyAction.RecoverAndVerify), int(bpp.VerifyAction.RecoverOnly))
    return [RV, V, RV, RO]


def _clip(bounds, c):
    return [b for b in bounds if b < c] + [c]


def _chunks(n, chunk):
    return list(range(0, n, chunk)) + [n]


def _outputs(e):
    e.wait()
    return (e.verdicts.cpu().numpy().copy(), e.masks.cpu().numpy().copy(), e.present.cpu().numpy().copy())


def _count_word(c):
    w = torch.tensor([c], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()  # (complete before any engine's stream reads it)
    return w


def _reference(packed, params, d, c, bounds, actions, m=1, proofs=None, weights=True):
    """a fresh upload of the first c items, the boundaries clipped to c: (verdicts, masks, present, weights of a blocking call)"""
    cb = _clip(bounds, c)
    rb = packed.ResidentBatch(params, _input(packed, d, c, m, proofs=proofs), None, None, None, None, LABEL, form="device")
    try:
        out = _outputs(rb.enqueue(bounds=cb, actions=actions[:len(cb) - 1]))
        w = None
        if weights:
            packed.verify_groups(rb, cb)
            w = np.frombuffer(rb.trace(3), dtype=np.uint8).reshape(c, 32).copy()
        return out + (w,)
    finally:
        rb.close()


@pytest.fixture(scope="module")
def references(bpp, packed, corpora):
    """(m, c) -> the reference of the clean corpus at count c, made on first use and never changed"""
    made = {}

    def get(m, c):
        if (m, c) not in made:
            params, d = corpora(m)
            if m == 1:
                made[(m, c)] = _reference(packed, params, d, c, BOUNDS, _actions(bpp))
            else:
                RV, RO = int(bpp.VerifyAction.RecoverAndVerify), int(bpp.VerifyAction.RecoverOnly)
                made[(m, c)] = _reference(packed, params, d, c, _chunks(N2, CHUNK2), [RO, RV, RO], m=2)
        return made[(m, c)]

    return get


def _empty_record(packed):
    return np.array([0, 0, 0, packed.VERDICT_WRITTEN | packed.VERDICT_EMPTY], dtype=np.int32)


def _hold(packed, got, want, bounds, c, what):
    """records of non-empty groups, mask rows and mask_present of live items: the reference's bytes; EMPTY records and zeros for the rest"""
    verdicts, masks, present = got[:3]
    live_groups = len(_clip(bounds, c)) - 1 if c else 0
    if c:
        assert verdicts[:live_groups].tobytes() == want[0].tobytes(), (what, c, verdicts, want[0])
        assert masks[:c].tobytes() == want[1].tobytes(), (what, c, "masks")
        assert present[:c].tobytes() == want[2].tobytes(), (what, c, "present")
    assert (verdicts[live_groups:] == _empty_record(packed)).all(), (what, c, verdicts)
    assert not masks[c:].any() and not present[c:].any(), (what, c, "dead slots")


def _secret_bytes(eng, handle=0):
    k = ctypes.c_uint64()
    assert eng.lib.bpp_batch_secret_bytes(eng.ctx, handle, ctypes.byref(k)) == 0
    return k.value


# ---- 1. one batch, every count, in sequence and shuffled; records, masks and weights
def test_every_count_equals_a_fresh_upload_of_the_first_items(bpp, packed, engine, corpora, references):
    params, d = corpora(1)
    actions = _actions(bpp)
    inp = _input(packed, d, N)
    rb = packed.ResidentBatch(params, inp, None, None, None, None, LABEL, form="device")
    order = COUNTS + [COUNTS[k] for k in np.random.default_rng(7).permutation(len(COUNTS))]
    assert any(a < b for a, b in zip(order[len(COUNTS):], order[len(COUNTS) + 1:])) and any(a > b for a, b in zip(order[len(COUNTS):], order[len(COUNTS) + 1:]))
    try:
        for c in order:
            filled = rb.refill(inp, count=_count_word(c))
            got = _outputs(rb.enqueue(bounds=BOUNDS, actions=actions))
            weights = rb.enqueue_weights().numpy()
            rec = filled.result()
            assert rec["flags"] == packed.REFILL_WRITTEN and rec["code"] == 0, (c, rec)
            want = references(1, c) if c else None
            _hold(packed, got, want, BOUNDS, c, "count")
            if c:  # valid proofs: every live group is Ok, and the masks are the openings' blinding factors where the group recovers
                assert (want[0][:, :3] == 0).all() and (want[0][:, 3] == packed.VERDICT_WRITTEN).all(), want[0]
                recovers = np.zeros(c, dtype=bool)
                for g in range(len(_clip(BOUNDS, c)) - 1):
                    if actions[g] != int(bpp.VerifyAction.VerifyOnly):
                        recovers[BOUNDS[g]:min(BOUNDS[g + 1], c)] = True
                assert got[2][:c].tolist() == recovers.astype(np.uint8).tolist(), c
                assert got[1][:c][recovers].tobytes() == d["blindings"][:c, 0][recovers].tobytes(), c
                # the cut chain: the reference's weights of the batch cut short
                assert weights[:c].tobytes() == want[3].tobytes(), (c, "weights")
                assert want[3].any(axis=1).all()
            assert not weights[c:].any(), (c, "dead weights")
    finally:
        rb.close()


# ---- 2. findings on either side of the count
def test_findings_below_the_count_are_reported_and_beyond_it_have_no_effect(bpp, packed, engine, corpora, references):
    params, d = corpora(1)
    actions = _actions(bpp)
    c = 134
    clean = _input(packed, d, N)
    rb = packed.ResidentBatch(params, clean, None, None, None, None, LABEL, form="device")

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
        # at and beyond the count, all four at once, and a missing nonce there: exactly the clean batch cut at c
        pr = tampered([c, c + 1, 250, N - 1])
        sp = np.ones(N, dtype=np.uint8)
        sp[c + 2] = 0
        filled = rb.refill(_input(packed, d, N, proofs=pr, seed_present=sp), count=_count_word(c))
        got = _outputs(rb.enqueue(bounds=BOUNDS, actions=actions))
        rec = filled.result()
        assert rec["flags"] == packed.REFILL_WRITTEN and rec["code"] == 0 and rec["msg"] == "", rec
        _hold(packed, got, references(1, c), BOUNDS, c, "findings beyond the count")
        assert (got[0][:3, :3] == 0).all()
        # below the count, what verification finds: the fresh upload's records (group 2 = [70, 134) verifies; group 0 recovers and verifies)
        for name, at, tier in (("invalid proof", [100, None, None, None], 7), ("identity member", [None, 3, None, None], 5),
                               ("both, in two groups", [133, 3, None, None], 7)):
            pr = tampered(at)
            inp = _input(packed, d, N, proofs=pr)
            filled = rb.refill(inp, count=_count_word(c))
            got = _outputs(rb.enqueue(bounds=BOUNDS, actions=actions))
            assert filled.result()["flags"] == packed.REFILL_WRITTEN, name
            want = _reference(packed, params, d, c, BOUNDS, actions, proofs=pr, weights=False)
            assert tier in want[0][:, 1].tolist(), (name, want[0])
            _hold(packed, got, want, BOUNDS, c, name)
        # below the count, what the upload refuses: its code and text, the lowest index; nothing of the verification is claimed
        pr = tampered([None, None, 90, None])
        pr[c + 5, S1:S1 + 32] = L_BYTES  # (a second one beyond the count changes nothing)
        filled = rb.refill(_input(packed, d, N, proofs=pr), count=_count_word(c))
        got = _outputs(rb.enqueue(bounds=BOUNDS, actions=actions))
        rec = filled.result()
        with pytest.raises(bpp.ProofError) as err:
            packed.ResidentBatch(params, _input(packed, d, c, proofs=pr), None, None, None, None, LABEL, form="device")
        assert rec["flags"] == packed.REFILL_WRITTEN | packed.REFILL_FINDING and rec["index"] == 90, rec
        assert rec["code"] == int(err.value.kind) and rec["msg"] == err.value.msg, (rec, err.value)
        want = np.array([rec["code"], 1, 90, packed.VERDICT_WRITTEN | packed.VERDICT_REFILL], dtype=np.int32)
        assert (got[0] == want).all() and not got[1].any() and not got[2].any(), got[0]
        pr = tampered([None, None, None, 7])
        filled = rb.refill(_input(packed, d, N, proofs=pr), count=_count_word(c))
        got = _outputs(rb.enqueue(bounds=BOUNDS, actions=actions))
        rec = filled.result()
        assert rec["flags"] == packed.REFILL_WRITTEN | packed.REFILL_FALLBACK and rec["code"] == 0, rec
        assert (got[0] == np.array([0, 0, 0, packed.VERDICT_WRITTEN | packed.VERDICT_REFILL], dtype=np.int32)).all(), got[0]
        # ... and the batch recovers
        rb.refill(clean, count=_count_word(c))
        _hold(packed, _outputs(rb.enqueue(bounds=BOUNDS, actions=actions)), references(1, c), BOUNDS, c, "clean again")
    finally:
        rb.close()


# ---- 3. secrets and reuse
def test_dead_slots_hold_no_nonce_and_come_back(bpp, packed, engine, corpora, references):
    params, d = corpora(1)
    actions = _actions(bpp)
    inp = _input(packed, d, N)
    rb = packed.ResidentBatch(params, inp, None, None, None, None, LABEL, form="device")
    try:
        assert np.count_nonzero(d["seeds"][70:]) > 0
        for c in (N, 70, 200, N):  # (the caller's array holds nonces in every slot)
            rb.refill(inp, count=_count_word(c))
            assert _secret_bytes(engine, rb.handle) == np.count_nonzero(d["seeds"][:c]), c
            got = _outputs(rb.enqueue(bounds=BOUNDS, actions=actions))
            _hold(packed, got, references(1, c), BOUNDS, c, "reuse")
    finally:
        rb.close()
    assert _secret_bytes(engine) == 0


# ---- 4. count handling
def test_count_beyond_the_batch_host_pointer_and_no_count(bpp, packed, corpora, references):
    _, d = corpora(1)
    actions = _actions(bpp)
    eng = bpp.Engine(0)
    params = bpp.RangeParameters.init(32, 1, bpp.create_pedersen_gens_with_extension_degree(1), engine=eng)
    inp = _input(packed, d, N)
    rb = packed.ResidentBatch(params, inp, None, None, None, None, LABEL, form="device")
    K = bpp.ProofErrorKind
    try:
        # a count in host memory: refused with the field named, nothing launched
        host = np.array([5], dtype=np.uint32)
        st = packed._lib.PackedBatch.from_buffer_copy(inp.struct)
        st.transcript_label, st.transcript_state, st.label_len = None, None, 0
        before = (packed.refill_stats(eng), packed.enqueue_stats(eng))
        rc = eng.lib.bpp_batch_refill_enqueue_count(eng.ctx, rb.handle, ctypes.byref(st), ctypes.c_void_p(host.ctypes.data), None, None)
        assert rc == int(K.InvalidArgument) and b"count_dev" in eng.lib.bpp_ctx_last_error(eng.ctx)
        assert (packed.refill_stats(eng), packed.enqueue_stats(eng)) == before
        rb.verify_only()  # (and the batch is still the host's)
        with pytest.raises(bpp.ProofError):
            rb.enqueue_weights()  # no enqueue yet
        # N + 1: BPP_REFILL_COUNT, nothing live, nothing claimed
        filled = rb.refill(inp, count=_count_word(N + 1))
        got = _outputs(rb.enqueue(bounds=BOUNDS, actions=actions))
        rec = filled.result()
        assert rec["flags"] == packed.REFILL_WRITTEN | packed.REFILL_COUNT and rec["code"] == 0 and rec["tier"] == 0 and "count" in rec["msg"], rec
        assert (got[0] == np.array([0, 0, 0, packed.VERDICT_WRITTEN | packed.VERDICT_REFILL], dtype=np.int32)).all(), got[0]
        assert not got[1].any() and not got[2].any() and not rb.enqueue_weights().numpy().any()
        assert _secret_bytes(eng, rb.handle) == 0
        # the next refill with a good count recovers
        rb.refill(inp, count=_count_word(135))
        _hold(packed, _outputs(rb.enqueue(bounds=BOUNDS, actions=actions)), references(1, 135), BOUNDS, 135, "after a bad count")
        # an empty group's text
        e = rb.enqueue(bounds=BOUNDS, actions=actions)
        res = e.results()
        assert res[3]["code"] == 0 and res[3]["tier"] == 0 and "no live item" in res[3]["msg"] and res[0]["msg"] == ""
        # one group over the whole batch (the one-group MSM plan), cut to five proofs and to none
        RV = bpp.VerifyAction.RecoverAndVerify
        one = references(1, 5)
        rb.refill(inp, count=_count_word(5))
        got = _outputs(rb.enqueue(action=RV))
        assert got[0].tolist() == [[0, 0, 0, packed.VERDICT_WRITTEN]] and got[1][:5].tobytes() == one[1].tobytes() and not got[1][5:].any()
        assert got[2].tolist() == [1] * 5 + [0] * (N - 5)
        rb.refill(inp, count=_count_word(0))
        got = _outputs(rb.enqueue(action=RV))
        assert (got[0] == _empty_record(packed)).all() and not got[1].any() and not got[2].any()
        # no count: bpp_batch_refill_enqueue, through the wrapper and through the new entry point with a null pointer
        full = references(1, N)
        rb.refill(inp)
        _hold(packed, _outputs(rb.enqueue(bounds=BOUNDS, actions=actions)), full, BOUNDS, N, "no count")
        assert rb.enqueue_weights().numpy().tobytes() == full[3].tobytes()
        rb.refill(inp, count=_count_word(1))
        assert eng.lib.bpp_batch_refill_enqueue_count(eng.ctx, rb.handle, ctypes.byref(st), None, None, None) == 0
        _hold(packed, _outputs(rb.enqueue(bounds=BOUNDS, actions=actions)), full, BOUNDS, N, "null count")
        with pytest.raises(bpp.ProofError) as e:
            rb.trace(3)
        assert e.value.kind == K.InvalidArgument and "upload the arrays for a blocking call" in str(e.value)
    finally:
        torch.cuda.synchronize()
        rb.close()
        params.close()
        eng.close()


def test_null_count_on_a_batch_that_never_took_one_equals_the_plain_refill(bpp, packed, engine, corpora, references):
    params, d = corpora(1)
    actions = _actions(bpp)
    inp = _input(packed, d, N)
    rb = packed.ResidentBatch(params, inp, None, None, None, None, LABEL, form="device")
    try:
        st = packed._lib.PackedBatch.from_buffer_copy(inp.struct)
        st.transcript_label, st.transcript_state, st.label_len = None, None, 0
        assert engine.lib.bpp_batch_refill_enqueue_count(engine.ctx, rb.handle, ctypes.byref(st), None, None, None) == 0
        a = _outputs(rb.enqueue(bounds=BOUNDS, actions=actions))
        wa = rb.enqueue_weights().numpy().tobytes()
        rb.refill(inp)
        b = _outputs(rb.enqueue(bounds=BOUNDS, actions=actions))
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
        _hold(packed, a, references(1, N), BOUNDS, N, "null count")
        assert wa == references(1, N)[3].tobytes() == rb.enqueue_weights().numpy().tobytes()
    finally:
        rb.close()


# ---- 5. the count is read on the stream, and only by the refill
def test_the_count_is_read_in_stream_order(bpp, packed, corpora, references):
    _, d = corpora(1)
    actions = _actions(bpp)
    want134, want70, want6 = references(1, 134), references(1, 70), references(1, 6)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        eng = bpp.Engine(0, stream=stream.cuda_stream)
        params = bpp.RangeParameters.init(32, 1, bpp.create_pedersen_gens_with_extension_degree(1), engine=eng)
        inp = packed.DevicePackedInput(_dev(d["proofs"]), _dev(d["commitments"]), _dev(d["min_values"]), _dev(d["min_present"]), _dev(d["seeds"]), LABEL)
        rb = packed.ResidentBatch(params, inp, None, None, None, None, LABEL, form="device")
        word = torch.zeros((1,), dtype=torch.int32, device="cuda")
        staged = torch.tensor([134, 999, 6, 3], dtype=torch.int32).pin_memory()
        rb.refill(inp, count=word)
        rb.enqueue(bounds=BOUNDS, actions=actions).wait()  # (the layout is planned here)
        r0, e0 = packed.refill_stats(eng), packed.enqueue_stats(eng)
        # from here on nothing waits: the word is written by a kernel just before the refill and overwritten just after it
        word.fill_(134)
        rb.refill(inp, count=word)
        word.fill_(999)
        first = rb.enqueue(bounds=BOUNDS, actions=actions)
        w_first = rb.enqueue_weights()
        second = rb.enqueue(bounds=BOUNDS, actions=actions)  # a later enqueue reads the batch's own word
        # ... by an asynchronous copy
        word.copy_(staged[2:3], non_blocking=True)
        rb.refill(inp, count=word)
        word.copy_(staged[3:4], non_blocking=True)
        third = rb.enqueue(bounds=BOUNDS, actions=actions)
        # ... and as an int, through the batch's own word
        rb.refill(inp, count=70)
        fourth = rb.enqueue(bounds=BOUNDS, actions=actions)
        rb.refill(inp, count=134)
        fifth = rb.enqueue(bounds=BOUNDS, actions=actions)
        r1, e1 = packed.refill_stats(eng), packed.enqueue_stats(eng)  # (before any wait)
        assert r1["host_waits"] == 0 and r1["calls"] == r0["calls"] + 4 and r1["first_calls"] == 1
        assert e1["host_waits"] == e0["host_waits"] and e1["layouts_in_call"] == e0["layouts_in_call"] and e1["calls"] == e0["calls"] + 5
        _hold(packed, _outputs(first), want134, BOUNDS, 134, "written before the refill")
        _hold(packed, _outputs(second), want134, BOUNDS, 134, "overwritten after the refill")
        assert w_first.numpy()[:134].tobytes() == want134[3].tobytes() and not w_first.numpy()[134:].any()
        _hold(packed, _outputs(third), want6, BOUNDS, 6, "an asynchronous copy")
        _hold(packed, _outputs(fourth), want70, BOUNDS, 70, "an int")
        _hold(packed, _outputs(fifth), want134, BOUNDS, 134, "an int again")
        assert word.cpu().tolist() == [3]
        rb.close()
        params.close()
        eng.close()


# ---- 6. aggregated proofs, equal chunks, actions per group
@pytest.mark.parametrize("c", COUNTS2)
def test_m2_chunks_with_actions(bpp, packed, engine, corpora, references, c):
    params, d = corpora(2)
    RV, RO = int(bpp.VerifyAction.RecoverAndVerify), int(bpp.VerifyAction.RecoverOnly)
    inp = _input(packed, d, N2, m=2)
    rb = packed.ResidentBatch(params, inp, None, None, None, None, LABEL, form="device")
    try:
        filled = rb.refill(inp, count=_count_word(c))
        got = _outputs(rb.enqueue(chunk=CHUNK2, actions=[RO, RV, RO]))
        weights = rb.enqueue_weights().numpy()
        assert filled.result()["flags"] == packed.REFILL_WRITTEN
        want = references(2, c) if c else None
        _hold(packed, got, want, _chunks(N2, CHUNK2), c, "m = 2")
        if c:
            assert (want[0][:, :3] == 0).all()
            assert weights[:c].tobytes() == want[3].tobytes()
        assert not weights[c:].any()
    finally:
        rb.close()
