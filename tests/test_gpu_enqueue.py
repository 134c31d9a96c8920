"""GPU tests: stream-ordered verification that leaves its verdicts on the device (bpp_verify_enqueue, csrc/verdict.h).

The reference in every comparison is the BLOCKING call on the same resident batch (verify_groups / verify_groups_actions), which the
rest of the suite holds to the oracle; the enqueue path is never compared against its own output.  One corpus of 600 proofs (64
bits, m = 1, seed nonces) serves every test."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from tests.helpers import LABEL

pytestmark = pytest.mark.gpu

BOUNDS = [0, 1, 8, 72, 272, 275, 600]
NONCANONICAL = np.frombuffer(b"\x01" + bytes(31), dtype=np.uint8)
A = slice(1 + 32, 1 + 64)  # the proof's A (t = 1: [t] d1 A A1 B r1 s1 ...)
R1 = 1 + 32 + 96           # first byte of r1: flipping a bit makes the final sum fail


@pytest.fixture(scope="module")
def packed():
    return importlib.import_module("bulletproofs-plus_amd.packed")


@pytest.fixture(scope="module")
def corpus(bpp, packed, engine):
    import bench
    params = bpp.RangeParameters.init(64, 1, bpp.create_pedersen_gens_with_extension_degree(1), engine=engine)
    d = bench.make_inputs(np, packed, params, 600, seed=8300)
    for a in d.values():
        if a is not None:
            a.setflags(write=False)
    yield params, d
    params.close()


def _resident(packed, params, d, proofs, sl=slice(None), seeds=True, form="packed"):
    return packed.ResidentBatch(params, proofs[sl], d["commitments"][sl], d["min_values"][sl], d["min_present"][sl],
                                d["seeds"][sl] if seeds else None, LABEL, form=form)


def _tampered(d):
    """the four tamperings of test_ragged_groups_equal_calls_of_their_own"""
    pr = d["proofs"].copy()
    pr[0, R1] ^= 1            # the one-proof group fails in its sum
    pr[100, A] = NONCANONICAL  # group 3 (72..271, across the 256 boundary): non-canonical A at in-group index 28
    pr[273, A] = 0            # group 4 (272..274): identity A at in-group index 1
    pr[274, A] = NONCANONICAL  # ... and a later-tier finding behind it
    return pr


def _same(got, want):
    assert len(got) == len(want)
    for g, (a, b) in enumerate(zip(got, want)):
        assert {k: a[k] for k in ("code", "tier", "index", "msg")} == {k: b[k] for k in ("code", "tier", "index", "msg")}, (g, a, b)


# ---- 1. precedence by class, and 7. the blocking paths are as they were
def test_precedence_by_class_equals_the_blocking_call(bpp, packed, engine, corpus):
    params, d = corpus
    cut = d["proofs"][:, :-64]  # every proof one (L, R) pair short: PASS 1 alone runs
    deg = d["proofs"].copy()    # a proof of another extension degree (t = 3, five pairs): nothing but the verdict kernels runs
    deg[5, 0] = 3
    deg[5, 1 + 32:1 + 96] = 0
    deg[5, 1 + 192:1 + 256] = 0
    edges = d["proofs"].copy()  # the boundaries of the binary search: last proof of one group, first proof of the next
    edges[71, A] = NONCANONICAL
    edges[72, A] = 0
    edges[599, R1] ^= 1
    waves = d["proofs"].copy()  # groups of 63, 64 and 65 proofs: the wavefront boundary, findings at their last proofs and beyond
    waves[62, A] = NONCANONICAL
    waves[63, R1] ^= 1
    waves[127 + 64, A] = 0
    wave_bounds = [0, 63, 127, 192, 600]
    seen_tiers = set()
    for proofs, cuts in ((d["proofs"], BOUNDS), (_tampered(d), BOUNDS), (cut, [0, 600]), (deg, [0, 600]), (edges, BOUNDS),
                         (waves, wave_bounds), (d["proofs"], wave_bounds)):
        rb = _resident(packed, params, d, proofs, seeds=False)
        want = packed.verify_groups(rb, cuts)
        before = packed.enqueue_stats(engine)
        e1 = rb.enqueue(bounds=cuts)
        e2 = rb.enqueue(bounds=cuts)  # the same layout again, behind the first: the stream orders them
        got2, got1 = e2.results(), e1.results()
        after = packed.enqueue_stats(engine)
        _same(got1, want)
        _same(got2, want)
        assert e1.done() and e2.done() and e1.redraws() == []
        assert int(e1.verdicts.cpu()[:, 3].min()) == packed.VERDICT_WRITTEN == int(e1.verdicts.cpu()[:, 3].max())
        assert after["calls"] - before["calls"] == 2 and after["groups"] - before["groups"] == 2 * (len(cuts) - 1)
        assert after["host_waits"] == before["host_waits"]
        seen_tiers |= {r["tier"] for r in want}
        # 7: status reset and layout reuse still hold for the blocking calls behind the enqueues
        _same(packed.verify_groups(rb, cuts), want)
        if proofs is d["proofs"]:
            rb.verify_only(64)
            _same(rb.enqueue(bounds=cuts).results(), want)  # (and back: a layout change with nothing in flight)
        rb.close()
    assert seen_tiers >= {0, 2, 5, 6, 7}  # (the corpus reaches Ok, DEGREE, PASS 1, PASS 2 and the MSM)


# ---- 2. actions and masks
def test_actions_and_masks_equal_the_blocking_call_byte_for_byte(bpp, packed, engine, corpus):
    params, d = corpus
    V, RV, RO = (int(bpp.VerifyAction.VerifyOnly), int(bpp.VerifyAction.RecoverAndVerify), int(bpp.VerifyAction.RecoverOnly))
    actions = [RV, V, RO, RV, RO, RV]
    pr = d["proofs"].copy()
    pr[100, R1] ^= 1  # group 3 (RecoverAndVerify) is rejected: rows zero and absent
    pr[50, R1] ^= 1   # group 2 (RecoverOnly) has a failing sum and still returns its masks
    rb = _resident(packed, params, d, pr)
    want, want_masks, want_present = packed.verify_groups_actions(rb, BOUNDS, actions)
    e = rb.enqueue(bounds=BOUNDS, actions=actions)
    _same(e.results(), want)
    masks, present = e.masks.cpu().numpy(), e.present.cpu().numpy()
    assert masks.tobytes() == want_masks.tobytes() and present.tobytes() == want_present.tobytes()
    assert want[3]["tier"] == 7 and not masks[72:272].any() and not present[72:272].any()
    assert want[2]["tier"] == 0 and present[8:72].all() and masks[8:72].any()
    assert masks[0:1].tobytes() == d["blindings"][0:1, 0].tobytes()  # (an accepted group's masks are the openings' blinding factors)
    assert not present[1:8].any()  # VerifyOnly
    # buffers the caller names, starting out as anything; and one action for every group
    verdicts = torch.full((len(BOUNDS) - 1, 4), -1, dtype=torch.int32, device="cuda")
    m2 = torch.full((600, 1, 32), 0xA5, dtype=torch.uint8, device="cuda")
    p2 = torch.full((600,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    e = rb.enqueue(bounds=BOUNDS, action=bpp.VerifyAction.RecoverOnly, verdicts=verdicts, masks=m2, present=p2)
    want, want_masks, want_present = packed.verify_groups_actions(rb, BOUNDS, [RO] * 6)
    _same(e.results(), want)
    assert e.verdicts is verdicts and m2.cpu().numpy().tobytes() == want_masks.tobytes() and p2.cpu().numpy().tobytes() == want_present.tobytes()
    rb.close()


# ---- 3. order without waits
def test_enqueues_of_several_batches_follow_each_other_without_a_wait(bpp, packed, corpus):
    params0, d = corpus
    eng = bpp.Engine(0)
    params = bpp.RangeParameters.init(64, 1, bpp.create_pedersen_gens_with_extension_degree(1), engine=eng)
    pr = d["proofs"].copy()
    pr[5 + 33, A] = NONCANONICAL  # the middle batch (proofs 5..74 of the corpus) is tampered
    cuts = [slice(0, 5), slice(5, 75), slice(75, 375)]
    bounds = [[0, 5], [0, 64, 70], [0, 256, 300]]
    rbs = [_resident(packed, params, d, pr, sl, seeds=False) for sl in cuts]
    want = [packed.verify_groups(rb, b) for rb, b in zip(rbs, bounds)]
    assert [r["tier"] for r in want[1]] == [6, 0]
    for rb in rbs:
        rb.close()
    for redraw in (False, True):
        rbs = [_resident(packed, params, d, pr, sl, seeds=False) for sl in cuts]  # fresh batches: their first enqueue lays them out
        before = packed.enqueue_stats(eng)
        out = []
        for _round in range(2):
            for k, (rb, b) in enumerate(zip(rbs, bounds)):
                if redraw and k == 1:
                    eng.set_option("chain_test_zero", 40)  # proof 39 of the middle batch is reported as a zero weight
                out.append(rb.enqueue(bounds=b))
                if redraw and k == 1:
                    eng.set_option("chain_test_zero", 0)
        after_enqueue = packed.enqueue_stats(eng)
        out[-1].wait()  # the one synchronisation
        after = packed.enqueue_stats(eng)
        assert after_enqueue["host_waits"] == before["host_waits"] == after["host_waits"]
        assert after["layouts_in_call"] - before["layouts_in_call"] == 3 and after["calls"] - before["calls"] == 6
        assert len({e.verdicts.data_ptr() for e in out}) == 6
        for i, e in enumerate(out):
            k = i % 3
            assert e.done()
            if redraw and k == 1:
                assert e.redraws() == [0, 1]
                host = e.verdicts.cpu().numpy()
                assert (host[:, :3] == 0).all() and (host[:, 3] == packed.VERDICT_WRITTEN | packed.VERDICT_REDRAW).all()
            else:
                assert e.redraws() == []
                _same(e.results(), want[k])
        if redraw:  # a blocking call on the middle batch afterwards gives the real verdict
            _same(packed.verify_groups(rbs[1], bounds[1]), want[1])
        for rb in rbs:
            rb.close()
    params.close()
    eng.close()


# ---- 4. chunk form
def test_chunk_form_equals_explicit_bounds(bpp, packed, engine, corpus):
    params, d = corpus
    pr = d["proofs"].copy()
    pr[300, R1] ^= 1
    pr[599, A] = NONCANONICAL
    rb = _resident(packed, params, d, pr, seeds=False)
    want = packed.verify_groups(rb, [0, 256, 512, 600])
    assert [r["tier"] for r in want] == [0, 7, 6]
    e = rb.enqueue(chunk=256)
    assert e.n_groups == 3 and tuple(e.verdicts.shape) == (3, 4)
    _same(e.results(), want)
    _same(rb.enqueue(bounds=[0, 256, 512, 600]).results(), want)
    rb.close()


# ---- 5. the caller's stream
def test_verdicts_are_consumed_on_the_producers_stream(bpp, packed, corpus):
    _, d = corpus
    n = 300
    src = {k: torch.from_numpy(d[k][:n].copy()).cuda() for k in ("proofs", "commitments", "min_present")}
    src["min_values"] = torch.from_numpy(d["min_values"][:n].copy().view(np.int64)).cuda()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        eng = bpp.Engine(0, stream=stream.cuda_stream)
        params = bpp.RangeParameters.init(64, 1, bpp.create_pedersen_gens_with_extension_degree(1), engine=eng)
        proofs = src["proofs"].clone()
        proofs[130, R1] ^= 1  # tampered by a torch operation on that stream: group 2 of [0, 64, 128, 192, 300]
        rb = packed.ResidentBatch(params, proofs, src["commitments"], src["min_values"], src["min_present"], None, LABEL, form="device")
        assert rb.input.synchronised is False
        e = rb.enqueue(bounds=[0, 64, 128, 192, 300])
        nonzero = (e.verdicts[:, 0] != 0).to(torch.int32)  # a torch reduction behind the call, on the same stream
        total = nonzero.sum()
        got = torch.stack([total, *nonzero]).cpu().tolist()  # .cpu() is the only synchronisation
        assert packed.enqueue_stats(eng)["host_waits"] == 0
        assert got == [1, 0, 0, 1, 0]
        rb.close()
        params.close()
        eng.close()


# ---- 6. refusals launch nothing
def test_refusals_launch_nothing(bpp, packed, corpus):
    """(The issue also lists a batch that hands out transcript states.  No upload makes one: the flag is set by the blocking
    bpp_verify_resident_states for the length of that call, under the context's lock, so no enqueue can meet it from outside; the
    engine refuses it all the same.)"""
    params0, d = corpus
    eng = bpp.Engine(0)
    params = bpp.RangeParameters.init(64, 1, bpp.create_pedersen_gens_with_extension_degree(1), engine=eng)
    rb = _resident(packed, params, d, d["proofs"], slice(0, 40))
    K = bpp.ProofErrorKind
    # (the HIP runtime this process has loaded, for one managed allocation that nothing ever touches)
    loaded = sorted({line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line})
    hip = ctypes.CDLL(loaded[0])
    managed = ctypes.c_void_p()
    assert hip.hipMallocManaged(ctypes.byref(managed), ctypes.c_size_t(4096), ctypes.c_uint(1)) == 0
    host = np.zeros(4096, dtype=np.uint8)
    dev = {"verdicts": torch.zeros((1, 4), dtype=torch.int32, device="cuda"), "masks": torch.zeros((40, 1, 32), dtype=torch.uint8, device="cuda"),
           "present": torch.zeros((40,), dtype=torch.uint8, device="cuda")}
    names = {"verdicts": "verdicts_dev", "masks": "masks_dev", "present": "mask_present_dev"}

    def refused(what, **kw):
        before = packed.enqueue_stats(eng)
        with pytest.raises(bpp.ProofError) as e:
            rb.enqueue(**kw)
        assert e.value.kind == K.InvalidArgument and what in str(e.value), (what, str(e.value))
        assert packed.enqueue_stats(eng) == before

    try:
        for field in ("verdicts", "masks", "present"):
            for bad in (host.ctypes.data, managed.value):
                refused(names[field], action=bpp.VerifyAction.RecoverAndVerify, **dict(dev, **{field: bad}))
        eng.set_option("verify_check", 1)
        refused("verify_check", **dev)
        eng.set_option("verify_check", -1)
        wide = dict(dev, verdicts=torch.zeros((3, 4), dtype=torch.int32, device="cuda"))
        refused("boundaries", bounds=[0, 10, 20, 39], **wide)
        refused("empty", bounds=[0, 10, 10, 40], **wide)
        before = packed.enqueue_stats(eng)
        e = rb.enqueue(action=bpp.VerifyAction.RecoverAndVerify, **dev)  # and the call itself still goes through
        assert [r["code"] for r in e.results()] == [0] and dev["present"].cpu().tolist() == [1] * 40
        assert packed.enqueue_stats(eng)["calls"] == before["calls"] + 1
    finally:
        torch.cuda.synchronize()
        hip.hipFree(managed)
        rb.close()
        params.close()
        eng.close()
