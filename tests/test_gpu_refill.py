"""GPU tests: a resident batch takes new contents of the same shape from device arrays on the stream (bpp_batch_refill_enqueue,
csrc/refill.h).

The reference in every comparison is a FRESH bpp_batch_upload_packed_device of the same arrays followed by bpp_verify_enqueue -- two
paths the rest of the suite holds to the host forms and the oracle (tests/test_gpu_device_inputs.py, tests/test_gpu_enqueue.py); a
refilled batch is never compared against its own output.  Where the fresh upload refuses the contents, its code and message are the
reference and the index is the lowest index the test tampered with (the blocking call's ABI returns no index; csrc/hosttest_refill.cpp
holds the record's index to the one the upload throws).  Proofs come from the engine's batch prover (bench.make_inputs), 32-bit
statements so that a promise can exceed the capacity."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from tests.helpers import LABEL

pytestmark = pytest.mark.gpu

L_BYTES = np.frombuffer(bytes.fromhex("edd3f55c1a631258d69cf7a2def9de14" + "00" * 15 + "10"), dtype=np.uint8)  # the group order
NOT_A_POINT = np.frombuffer(b"\x01" + bytes(31), dtype=np.uint8)
R1 = 1 + 32 + 96  # t = 1: [t] d1 A A1 B r1 s1 (L R)*
S1 = R1 + 32
TIER_CONSTRUCTION = 1


@pytest.fixture(scope="module")
def packed():
    return importlib.import_module("bulletproofs-plus_amd.packed")


@pytest.fixture(scope="module")
def corpora(bpp, packed, engine):
    """m -> (params, arrays of 300 proofs at 32 bits), made once and never changed (tests work on copies)"""
    import bench
    made = {}

    def get(m):
        if m not in made:
            params = bpp.RangeParameters.init(32, m, bpp.create_pedersen_gens_with_extension_degree(1), engine=engine)
            d = bench.make_inputs(np, packed, params, 300 if m == 1 else 17, seed=9400 + m)
            if d["seeds"] is None:  # (m = 2: the recipe makes none; a nonce array that no item uses still shapes the batch)
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
        a = a.copy()  # (the corpus is read-only; torch wants a writable source)
    if a.dtype == np.uint64:
        a = a.view(np.int64)  # torch's uint64 is thin: the bit patterns travel as int64
    return torch.from_numpy(a).cuda()


def _input(packed, d, n, off, nonces, proofs=None, commitments=None, min_values=None, seed_present=None, gap=0xEE):
    """the first n items as a DevicePackedInput whose proofs start `off` bytes into their allocation, rows proof_len + 5 apart;
    nonces: "none", "all" or "some" (through seed_present; an explicit seed_present overrides)"""
    proofs = (d["proofs"] if proofs is None else proofs)[:n]
    plen, stride = proofs.shape[1], proofs.shape[1] + 5
    flat = np.full(off + n * stride, gap, dtype=np.uint8)
    np.lib.stride_tricks.as_strided(flat[off:], shape=(n, plen), strides=(stride, 1))[:] = proofs
    base = torch.from_numpy(flat).cuda()
    view = torch.as_strided(base, (n, plen), (stride, 1), off)
    seeds = None if nonces == "none" else _dev(d["seeds"][:n])
    if seed_present is None and nonces == "some":
        seed_present = (np.arange(n) % 3 == 1).astype(np.uint8)
    if seed_present is None and nonces == "nobody":
        seed_present = np.zeros(n, dtype=np.uint8)
    inp = packed.DevicePackedInput(view, _dev((d["commitments"] if commitments is None else commitments)[:n]),
                                   _dev((d["min_values"] if min_values is None else min_values)[:n]), _dev(d["min_present"][:n]), seeds, LABEL,
                                   seed_present=_dev(seed_present), proof_stride=stride if n == 1 else None)
    assert inp.struct.proof_stride == stride
    torch.cuda.synchronize()  # (the arrays are complete before any engine's stream reads them)
    return inp


def _groups(bpp, n):
    """three unequal groups with mixed actions (one group for a batch of one)"""
    V, RV, RO = (int(bpp.VerifyAction.VerifyOnly), int(bpp.VerifyAction.RecoverAndVerify), int(bpp.VerifyAction.RecoverOnly))
    if n == 1:
        return [0, 1], [RV]
    cut1 = max(1, n // 5)
    cut2 = min(n - 1, max(cut1 + 1, n - n // 7 - 1))
    return [0, cut1, cut2, n], [RV, V, RO]


def _outputs(e):
    e.wait()
    return (e.verdicts.cpu().numpy().copy(), e.masks.cpu().numpy().copy(), e.present.cpu().numpy().copy())


def _fresh(packed, params, inp, bounds, actions):
    """the reference: a fresh upload of the same arrays, one enqueue"""
    rb = packed.ResidentBatch(params, inp, None, None, None, None, LABEL, form="device")
    try:
        return _outputs(rb.enqueue(bounds=bounds, actions=actions))
    finally:
        rb.close()


SHAPES = [(1, 300, 3, "all"), (1, 17, 0, "some"), (1, 1, 1, "none"), (2, 17, 1, "nobody")]


# ---- 1. one batch, a sequence of refills
@pytest.mark.parametrize("m,n,off,nonces", SHAPES)
def test_a_sequence_of_refills_equals_fresh_uploads(bpp, packed, engine, corpora, m, n, off, nonces):
    params, d = corpora(m)
    bounds, actions = _groups(bpp, n)
    last = n - 1
    K = bpp.ProofErrorKind

    def tampered(rows):
        pr = d["proofs"][:n].copy()
        for i, at, value in rows:
            pr[i, at:at + 32] = value
        return pr

    invalid = d["proofs"][:n].copy()
    invalid[0, R1] ^= 1  # (group 0 recovers AND verifies: its final sum fails)
    bad_commit = d["commitments"][:n].copy()
    bad_commit[n // 2, m - 1] = NOT_A_POINT
    over = d["min_values"][:n].copy()
    over[n // 3, 0] = 1 << 32
    foreign = d["proofs"][:n].copy()
    foreign[n // 2, 0] = 2
    # (name, keyword arguments of _input, the fresh upload's finding index or None, tier the reference must reach or None)
    steps = [("clean", {}, None, 0),
             ("invalid proof", {"proofs": invalid}, None, 7),
             ("commitment does not decode", {"commitments": bad_commit}, None, 4),
             ("promise over capacity", {"min_values": over}, None, 3),
             ("non-canonical scalar at index 0", {"proofs": tampered([(0, R1, L_BYTES)])}, 0, None),
             ("non-canonical scalar at the last index", {"proofs": tampered([(last, S1, L_BYTES)])}, last, None),
             ("two findings", {"proofs": tampered([(last, 1, L_BYTES), (n // 2, S1, L_BYTES)])}, n // 2 if n > 1 else 0, None),
             ("garbage between the rows", {"gap": 0x10}, None, 0),
             ("one foreign first byte", {"proofs": foreign}, "fallback", None)]
    if m == 2:
        only = np.zeros(n, dtype=np.uint8)
        only[5] = 1
        steps.append(("a nonce with m = 2", {"seed_present": only}, 5, None))
    steps.append(("clean again", {}, None, 0))

    rb = packed.ResidentBatch(params, _input(packed, d, n, off, nonces), None, None, None, None, LABEL, form="device")
    try:
        for name, kw, finding, tier in steps:
            inp = _input(packed, d, n, off, nonces, **kw)
            filled = rb.refill(inp)
            got = _outputs(rb.enqueue(bounds=bounds, actions=actions))
            rec = filled.result()
            if finding is None:
                want = _fresh(packed, params, inp, bounds, actions)
                assert rec["flags"] == packed.REFILL_WRITTEN and rec["code"] == 0, (name, rec)
                for a, b, what in zip(got, want, ("verdicts", "masks", "present")):
                    assert a.tobytes() == b.tobytes(), (name, what, a[:4], b[:4])
                tiers = set(want[0][:, 1].tolist())
                assert tier in tiers and (tier != 0 or tiers == {0}), (name, want[0])
                assert (want[0][:, 3] == packed.VERDICT_WRITTEN).all()
                if tier == 0 and nonces in ("all", "some") and m == 1:  # the right masks: the openings' blinding factors
                    present = np.zeros(n, dtype=np.uint8)
                    lo, hi = bounds[0], bounds[1]
                    present[lo:hi] = 1 if nonces == "all" else (np.arange(lo, hi) % 3 == 1)
                    present[bounds[2]:] = 1 if nonces == "all" else (np.arange(bounds[2], n) % 3 == 1)
                    assert got[2].tolist() == present.tolist(), name
                    assert got[1][present == 1].tobytes() == d["blindings"][:n, 0][present == 1].tobytes(), name
                    assert not got[1][present == 0].any(), name
                continue
            # contents the blocking upload does not take as they are: nothing of the verification is claimed, no masks
            assert not got[1].any() and not got[2].any(), name
            before = packed.ingest_stats(engine)
            if finding == "fallback":
                assert rec["flags"] == packed.REFILL_WRITTEN | packed.REFILL_FALLBACK and rec["code"] == 0 and rec["tier"] == 0, (name, rec)
                assert (got[0] == np.array([0, 0, 0, packed.VERDICT_WRITTEN | packed.VERDICT_REFILL], dtype=np.int32)).all(), (name, got[0])
                try:  # the blocking upload stages such a batch and takes the host path (whatever that comes to)
                    packed.ResidentBatch(params, inp, None, None, None, None, LABEL, form="device").close()
                except bpp.ProofError:
                    pass
                after = packed.ingest_stats(engine)
                if n > 1:  # (a batch of one cannot disagree with itself: to a fresh upload the byte is simply another shape)
                    assert after[1] == before[1] + 1 and after[0] == before[0], name
                continue
            with pytest.raises(bpp.ProofError) as err:
                packed.ResidentBatch(params, inp, None, None, None, None, LABEL, form="device")
            assert rec["flags"] == packed.REFILL_WRITTEN | packed.REFILL_FINDING and rec["tier"] == TIER_CONSTRUCTION, (name, rec)
            assert rec["code"] == int(err.value.kind) and rec["msg"] == err.value.msg and rec["index"] == finding, (name, rec, err.value)
            want = np.array([rec["code"], TIER_CONSTRUCTION, finding, packed.VERDICT_WRITTEN | packed.VERDICT_REFILL], dtype=np.int32)
            assert (got[0] == want).all(), (name, got[0])
            if name == "two findings" and n > 1:
                assert rec["msg"] == "Invalid parsing" and rec["code"] == int(K.InvalidArgument)
    finally:
        rb.close()


# ---- 2. no host involvement
def test_steady_state_has_no_host_involvement(bpp, packed, corpora):
    _, d = corpora(1)
    eng = bpp.Engine(0)
    params = bpp.RangeParameters.init(32, 1, bpp.create_pedersen_gens_with_extension_degree(1), engine=eng)
    n, (bounds, actions) = 300, _groups(bpp, 300)
    invalid = d["proofs"][:n].copy()
    invalid[40, R1] ^= 1
    ring = [_input(packed, d, n, 1, "all"), _input(packed, d, n, 1, "all", proofs=invalid)]
    rb = packed.ResidentBatch(params, ring[0], None, None, None, None, LABEL, form="device")
    try:
        want = [_fresh(packed, params, inp, bounds, actions) for inp in ring]
        assert want[0][0][:, 1].tolist() == [0, 0, 0] and want[1][0][:, 1].tolist() == [7, 0, 0]
        rb.refill(ring[1])
        rb.enqueue(bounds=bounds, actions=actions).wait()
        r0, e0 = packed.refill_stats(eng), packed.enqueue_stats(eng)
        assert r0 == {"calls": 1, "first_calls": 1, "host_waits": 0}
        out = []
        for k in range(20):
            rb.refill(ring[k % 2])
            out.append(rb.enqueue(bounds=bounds, actions=actions))
        r1, e1 = packed.refill_stats(eng), packed.enqueue_stats(eng)  # (before any wait: nothing was waited for to get here)
        assert r1 == {"calls": 21, "first_calls": 1, "host_waits": 0}
        assert e1["layouts_in_call"] == e0["layouts_in_call"] and e1["host_waits"] == e0["host_waits"] and e1["calls"] == e0["calls"] + 20
        for k, e in enumerate(out):
            for a, b in zip(_outputs(e), want[k % 2]):
                assert a.tobytes() == b.tobytes(), k
    finally:
        rb.close()
        params.close()
        eng.close()


# ---- 3. producer and consumer on one stream
def test_producer_refill_enqueue_and_consumer_on_one_stream(bpp, packed, corpora):
    _, d = corpora(1)
    n, bounds = 300, [0, 64, 128, 192, 300]
    tampered = d["proofs"][:n].copy()
    tampered[130, R1] ^= 1   # group 2: the final sum fails
    tampered[250, 1 + 32:1 + 64] = 0  # group 3: identity A, a PASS-1 finding
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        eng = bpp.Engine(0, stream=stream.cuda_stream)
        params = bpp.RangeParameters.init(32, 1, bpp.create_pedersen_gens_with_extension_degree(1), engine=eng)
        blocking = packed.ResidentBatch(params, tampered, d["commitments"][:n], d["min_values"][:n], d["min_present"][:n], None, LABEL)
        want = [int(r["code"] != 0) for r in packed.verify_groups(blocking, bounds)]
        blocking.close()
        assert want == [0, 0, 1, 1]
        staging = _dev(tampered)
        slot = _dev(d["proofs"][:n])  # the buffer the batch is refilled from: clean proofs for now
        inp = packed.DevicePackedInput(slot, _dev(d["commitments"][:n]), _dev(d["min_values"][:n]), _dev(d["min_present"][:n]), None, LABEL)
        rb = packed.ResidentBatch(params, inp, None, None, None, None, LABEL, form="device")
        rb.refill(inp)
        assert [r["code"] for r in rb.enqueue(bounds=bounds).results()] == [0, 0, 0, 0]  # (the layout is planned here)
        before = packed.enqueue_stats(eng)
        # from here on everything is on `stream` and nothing waits: producer, refill, verification, consumer
        slot.copy_(staging, non_blocking=True)
        rb.refill(inp)
        e = rb.enqueue(bounds=bounds)
        nonzero = (e.verdicts[:, 0] != 0).to(torch.int32)
        total = nonzero.sum()
        got = torch.stack([total, *nonzero]).cpu().tolist()  # .cpu() is the only synchronisation
        after = packed.enqueue_stats(eng)
        assert got == [sum(want)] + want
        assert packed.refill_stats(eng) == {"calls": 2, "first_calls": 1, "host_waits": 0}
        assert after["host_waits"] == before["host_waits"] and after["layouts_in_call"] == before["layouts_in_call"]
        rb.close()
        params.close()
        eng.close()


# ---- 4. secrets
def _secret_bytes(eng, handle=0):
    k = ctypes.c_uint64()
    assert eng.lib.bpp_batch_secret_bytes(eng.ctx, handle, ctypes.byref(k)) == 0
    return k.value


def test_a_refill_without_nonces_leaves_no_secret_behind(bpp, packed, engine, corpora):
    params, d = corpora(1)
    n = 17
    rb = packed.ResidentBatch(params, _input(packed, d, n, 0, "all"), None, None, None, None, LABEL, form="device")
    try:
        rb.refill(_input(packed, d, n, 3, "all"))
        e = rb.enqueue(action=bpp.VerifyAction.RecoverAndVerify)
        assert [r["code"] for r in e.results()] == [0] and e.present.cpu().tolist() == [1] * n
        assert e.masks.cpu().numpy().tobytes() == d["blindings"][:n, 0].tobytes()
        assert _secret_bytes(engine, rb.handle) > 2 * n * 24  # nonces + masks
        filled = rb.refill(_input(packed, d, n, 3, "nobody"))
        assert filled.result()["flags"] == packed.REFILL_WRITTEN
        assert _secret_bytes(engine, rb.handle) == 0
        e = rb.enqueue(action=bpp.VerifyAction.RecoverAndVerify)
        assert [r["code"] for r in e.results()] == [0] and not e.present.cpu().any() and not e.masks.cpu().any()
        assert _secret_bytes(engine, rb.handle) == 0
    finally:
        rb.close()
    assert _secret_bytes(engine) == 0


# ---- 5. refusals launch nothing
def test_refusals_launch_nothing(bpp, packed, corpora):
    _, d = corpora(1)
    _, d2 = corpora(2)
    eng = bpp.Engine(0)
    params = bpp.RangeParameters.init(32, 1, bpp.create_pedersen_gens_with_extension_degree(1), engine=eng)
    n = 17
    K = bpp.ProofErrorKind
    good = _input(packed, d, n, 0, "all")
    rb = packed.ResidentBatch(params, good, None, None, None, None, LABEL, form="device")
    record = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    host = np.zeros(1 << 16, dtype=np.uint8)

    def refused(what, inp, target=None, **kw):
        before = (packed.refill_stats(eng), packed.enqueue_stats(eng))
        with pytest.raises(bpp.ProofError) as e:
            (target or rb).refill(inp, **dict({"record": record}, **kw))
        assert e.value.kind == K.InvalidArgument and what in str(e.value), (what, str(e.value))
        assert (packed.refill_stats(eng), packed.enqueue_stats(eng)) == before

    def arrays(**kw):
        a = {"proofs": _dev(d["proofs"][:n]), "commitments": _dev(d["commitments"][:n]), "min_values": _dev(d["min_values"][:n]),
             "min_present": _dev(d["min_present"][:n]), "seed_nonces": _dev(d["seeds"][:n]), "seed_present": None}
        a.update(kw)
        return packed.DevicePackedInput(a["proofs"], a["commitments"], a["min_values"], a["min_present"], a["seed_nonces"], LABEL,
                                        seed_present=a["seed_present"])

    try:
        # a shape field that differs, each in turn
        refused("n_items", _input(packed, d, n - 1, 0, "all"))
        refused("m differs", arrays(proofs=_dev(d["proofs"][:n]), commitments=_dev(d2["commitments"][:n]), min_values=_dev(d2["min_values"][:n]),
                                    min_present=_dev(d2["min_present"][:n])))
        refused("proof_len", arrays(proofs=_dev(d["proofs"][:n, :-64])))
        refused("seed_nonces32", arrays(seed_nonces=None))
        refused("min_values", arrays(min_values=None, min_present=None))
        refused("min_present", arrays(min_present=None))
        short = arrays()
        short.struct.proof_stride = short.struct.proof_len - 1
        refused("proof_stride", short)
        # a transcript field (the wrapper clears them: the C call itself)
        for field in ("transcript_label", "transcript_state"):
            st = packed._lib.PackedBatch.from_buffer_copy(good.struct)
            st.transcript_label, st.transcript_state = None, None
            setattr(st, field, host.ctypes.data)
            before = packed.refill_stats(eng)
            assert eng.lib.bpp_batch_refill_enqueue(eng.ctx, rb.handle, ctypes.byref(st), None, None) == int(K.InvalidArgument)
            assert b"transcript" in eng.lib.bpp_ctx_last_error(eng.ctx) and packed.refill_stats(eng) == before
        # a host pointer for each array and for the record
        plen = d["proofs"].shape[1]
        for field, shape in (("proofs", (n, plen)), ("commitments", (n, 1, 32)), ("min_values", (n, 1)), ("min_present", (n, 1)),
                             ("seed_nonces", (n, 32)), ("seed_present", (n,))):
            name = {"commitments": "commitments32", "seed_nonces": "seed_nonces32"}.get(field, field)
            refused(name + ":", arrays(**{field: (host.ctypes.data, shape)}))
        refused("record_dev", good, record=host.ctypes.data)
        # batches of another origin
        for form in ("packed", "items"):
            other = packed.ResidentBatch(params, d["proofs"][:n], d["commitments"][:n], d["min_values"][:n], d["min_present"][:n], d["seeds"][:n],
                                         LABEL, form=form)
            refused("cannot be refilled", good, target=other)
            other.verify_only()  # (and it stays what it was)
            other.close()
        assert eng.lib.bpp_batch_refill_enqueue(eng.ctx, ctypes.c_uint64(1 << 60), ctypes.byref(good.struct), None, None) == -3
        torch.cuda.synchronize()
        assert record.cpu().tolist() == [-7] * 4 and packed.refill_stats(eng) == {"calls": 0, "first_calls": 0, "host_waits": 0}
        # the call itself goes through, and the batch is the stream's from then on
        rb.verify_only()
        filled = rb.refill(good, record=record)
        assert filled.result()["flags"] == packed.REFILL_WRITTEN and filled.record is record
        assert [r["code"] for r in rb.enqueue().results()] == [0]
        before = (packed.refill_stats(eng), packed.enqueue_stats(eng))
        for call in (rb.verify_only, lambda: rb.verify_arrays(bpp.VerifyAction.RecoverOnly), lambda: packed.verify_groups(rb, [0, n]),
                     rb.phase1, lambda: rb.trace(2)):
            with pytest.raises(bpp.ProofError) as e:
                call()
            assert e.value.kind == K.InvalidArgument and "upload the arrays for a blocking call" in str(e.value)
        assert (packed.refill_stats(eng), packed.enqueue_stats(eng)) == before
        assert rb.shape()["n_items"] == n and _secret_bytes(eng, rb.handle) > 0  # shape and secret_bytes keep working, destroy below
    finally:
        torch.cuda.synchronize()
        rb.close()
        params.close()
        eng.close()
