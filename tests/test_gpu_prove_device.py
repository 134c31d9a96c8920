"""GPU tests of proving from openings that lie in device memory (bpp_prove_openings_device): for any input the call writes what
bpp_prove_openings writes on the equivalent bpp_prove_item array over host copies of the same arrays -- return code, message,
per-item codes, lengths, proof and commitment bytes, the zeroed slots of failed items -- with the proofs and commitments left in
device memory, in the row geometry the mixed device upload and refill take as they are.  The reference of every comparison is
bpp_prove_openings on the same engine; the oracle (oracle.cport / oracle.pyref) is the reference for a few items besides.  Input
slack holds 0xFF (a finding if it were read), the outputs are prefilled with 0xA5 in both forms and compared as whole buffers, so
every comparison is also the statement that no slack byte was written."""
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
INVALID_ARGUMENT, INVALID_LENGTH = 2, 3
PATTERN = [1, 4, 2, 8, 1]
L_ORDER = 2 ** 252 + 27742317777372353535851937790883648493
_CACHE = {}


def _params(bpp, engine, t, n_bits=N):
    if (t, n_bits) not in _CACHE:
        _CACHE[(t, n_bits)] = bpp.RangeParameters.init(n_bits, M_MAX, bpp.create_pedersen_gens_with_extension_degree(t), engine=engine)
    return _CACHE[(t, n_bits)]


def _rounds(m, n_bits=N):
    return (n_bits * m).bit_length() - 1


def _plen(m, t, n_bits=N):
    return 1 + 32 * (t + 5 + 2 * _rounds(m, n_bits))


def _state():
    t0 = M.Transcript(b"outer protocol")
    t0.append_message(b"ctx", b"openings on the device")
    return t0


def _scalars(rng, shape):
    a = rng.integers(0, 256, size=tuple(shape) + (32,), dtype=np.uint8)
    a[..., 31] &= 0x0F  # < 2^252 < l
    return a


def _data(t, ms, seed, n_bits=N, promises=True, nonces=True, rng_slack=8):
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
    d["rng"] = np.full((n, 32 * (_rounds(M_MAX, n_bits) + 3) + rng_slack), 0xFF, dtype=np.uint8)
    for i, m in enumerate(ms):
        if m not in (1, 2, 4, 8):
            continue
        d["values"][i, :m] = rng.integers(0, 2 ** (n_bits - 1), size=m, dtype=np.uint64)
        d["blind"][i, :m] = _scalars(rng, (m, t))
        d["minp"][i, :m] = [(i + j) % 2 == 0 and promises for j in range(m)]
        d["minv"][i, :m] = d["values"][i, :m] // 3
        if nonces and m == 1:
            d["seeds"][i] = _scalars(rng, ())
            d["seedp"][i] = 1
        need = 32 * (_rounds(m, n_bits) + 3)
        d["rng"][i, :need] = rng.integers(0, 256, size=need, dtype=np.uint8)
    d["commit"], d["state"], d["label"] = None, None, LABEL
    return d


def _host(engine, params, packed, d, pstride, cstride, rng_stride=None):
    """bpp_prove_openings on the equivalent items over the host arrays -> dict(rc, msg, codes, lens, proofs, commits, texts)"""
    n, t = d["n"], d["t"]
    keep = {k: np.ascontiguousarray(d[k]) for k in ("values", "blind", "minv", "minp", "seeds", "rng")}
    items = np.zeros(n, dtype=packed._PROVE_ITEM)
    items["values"] = packed._rows(keep["values"])
    items["blindings32"] = packed._rows(keep["blind"])
    if d["commit"] is not None:
        keep["commit"] = np.ascontiguousarray(d["commit"])
        items["commitments32"] = packed._rows(keep["commit"])
    items["m"] = d["m"]
    if d.get("promise_arrays", True):
        items["min_values"] = packed._rows(keep["minv"])
        items["min_present"] = packed._rows(keep["minp"])
    if d.get("nonce_array", True):
        items["seed_nonce32"] = np.where(d["seedp"] != 0, packed._rows(keep["seeds"]), np.uint64(0))
    lbl = np.frombuffer(d["label"], dtype=np.uint8).copy()
    if d["state"] is not None:
        st = np.frombuffer(d["state"], dtype=np.uint8).copy()
        items["transcript_state"] = st.ctypes.data
    else:
        items["transcript_label"] = lbl.ctypes.data
        items["label_len"] = len(d["label"])
    items["rng_bytes"] = packed._rows(keep["rng"])
    items["rng_len"] = keep["rng"].shape[1] if rng_stride is None else rng_stride
    proofs = np.full((n, pstride), 0xA5, dtype=np.uint8)
    commits = np.full((n, cstride), 0xA5, dtype=np.uint8)
    lens = np.zeros(n, dtype=np.uintp)
    codes = np.zeros(n, dtype=np.intc)
    err = ctypes.create_string_buffer(256)
    arr = items.ctypes.data_as(ctypes.POINTER(packed._lib.ProveItem))
    rc = engine.lib.bpp_prove_openings(engine.ctx, params.handle, arr, n, commits.ctypes.data, cstride, proofs.ctypes.data, pstride,
                                       lens.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t)), codes.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), err, 256)
    texts = []
    for i in range(n):
        buf = ctypes.create_string_buffer(256)
        engine.lib.bpp_prove_openings_item_message(engine.ctx, params.handle, ctypes.byref(arr[i]), None, cstride, pstride, int(codes[i]), buf, 256)
        texts.append(buf.value.decode())
    return dict(rc=rc, msg=err.value.decode(), codes=codes, lens=lens, proofs=proofs, commits=commits, texts=texts)


def _dev(a):
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _openings(packed, d, rng_view=None):
    rng_bytes = _dev(d["rng"]) if rng_view is None else rng_view
    promise = d.get("promise_arrays", True)
    nonce = d.get("nonce_array", True)
    return packed.DeviceOpenings(_dev(d["values"]), _dev(d["blind"]), d["m"], commitments=None if d["commit"] is None else _dev(d["commit"]),
                                 min_values=_dev(d["minv"]) if promise else None, min_present=_dev(d["minp"]) if promise else None,
                                 seed_nonces=_dev(d["seeds"]) if nonce else None, seed_present=_dev(d["seedp"]) if nonce else None,
                                 rng_bytes=rng_bytes, label=d["label"], state=d["state"])


def _device(engine, params, packed, d, pstride, cstride, inp=None):
    inp = _openings(packed, d) if inp is None else inp
    proofs = torch.full((d["n"], pstride), 0xA5, dtype=torch.uint8, device="cuda")
    commits = torch.full((d["n"], cstride), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return packed.prove_openings_device(params, inp, commitments_out=commits, proofs_out=proofs)


def _same(engine, res, ref, rows=True):
    """everything the contract names, whole buffers: slack included (rows=False: all but the output rows)"""
    assert res.rc == ref["rc"] and res.message == ref["msg"], (res.rc, res.message, ref["rc"], ref["msg"])
    assert list(res.codes) == list(ref["codes"])
    assert list(res.proof_lens) == list(ref["lens"])
    got_p, got_c = res.proofs.cpu().numpy(), res.commitments.cpu().numpy()
    bad = [i for i in range(len(ref["codes"])) if not (np.array_equal(got_p[i], ref["proofs"][i]) and np.array_equal(got_c[i], ref["commits"][i]))]
    assert not (rows and bad), "rows %s differ from bpp_prove_openings on host copies of the same arrays" % bad[:8]
    st = res.status.cpu().numpy()
    assert list(st[:, 0]) == list(ref["codes"])
    assert [m for _, m in res.messages(engine)] == ref["texts"]


def _no_secrets_left(engine):
    examined, nonzero = ctypes.c_uint64(), ctypes.c_uint64()
    assert engine.lib.bpp_prove_secret_bytes(engine.ctx, ctypes.byref(examined), ctypes.byref(nonzero)) == 0
    assert examined.value > 0 and nonzero.value == 0


def _oracle(d, i, cp):
    m, t = int(d["m"][i]), d["t"]
    vals = [int(v) for v in d["values"][i, :m]]
    blinds = [[bytes(d["blind"][i, j, k]) for k in range(t)] for j in range(m)]
    mins = [int(d["minv"][i, j]) if d["minp"][i, j] else None for j in range(m)]
    nonce = bytes(d["seeds"][i]) if d["seedp"][i] else None
    ext = bytes(d["rng"][i, :32 * (_rounds(m) + 3)])
    if d["state"] is None:
        proof, comms = cp.prove(d["label"], vals, blinds, mins, nonce, ext)
        return b"".join(bytes(c) for c in comms), proof
    comms = [cp.commit(vals[j], blinds[j]) for j in range(m)]
    op = O.RangeParameters(N, M_MAX, O.PedersenGens(t))
    ost = O.RangeStatement(op, [C.decompress(c) for c in comms], mins, None if nonce is None else int.from_bytes(nonce, "little"))
    ow = O.RangeWitness([O.CommitmentOpening(vals[j], [int.from_bytes(x, "little") for x in blinds[j]]) for j in range(m)])
    assert d["state"] == _state().strobe.to_bytes()
    return b"".join(bytes(c) for c in comms), O.prove_with_rng(_state(), ost, ow, M.ByteStreamRng(ext)).to_bytes()


def _against_oracle(d, res, which):
    cp = cport.Params(N, M_MAX, d["t"])
    got_p, got_c = res.proofs.cpu().numpy(), res.commitments.cpu().numpy()
    for i in which:
        comms, proof = _oracle(d, i, cp)
        assert bytes(got_c[i, :len(comms)]) == comms, "commitments of item %d differ from the oracle's" % i
        assert bytes(got_p[i, :int(res.proof_lens[i])]) == proof, "proof %d differs from the oracle prover's" % i
    cp.close()


# ---------------------------------------------------------------- 1. one item
def test_one_item(bpp, engine):
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    params = _params(bpp, engine, 1)
    d = _data(1, [1], 1, nonces=False)
    ps, cs = _plen(1, 1) + 7, 32 * MS
    res = _device(engine, params, packed, d, ps, cs)
    assert res.rc == 0, res.message
    _same(engine, res, _host(engine, params, packed, d, ps, cs))
    _against_oracle(d, res, [0])


# ---------------------------------------------------------------- 2. mixed, unsorted; 9. secrets
def test_mixed_unsorted_under_a_transcript_state(bpp, engine):
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    params = _params(bpp, engine, 3)
    d = _data(3, PATTERN, 2)
    d["state"] = _state().strobe.to_bytes()
    ps, cs = _plen(8, 3) + 7, 32 * MS
    res = _device(engine, params, packed, d, ps, cs)
    assert res.rc == 0 and not any(res.codes), res.message
    _same(engine, res, _host(engine, params, packed, d, ps, cs))
    _against_oracle(d, res, [0, 2])
    _no_secrets_left(engine)


# ---------------------------------------------------------------- 3. two sub-batches; 10. round trip; 11. existing calls untouched
def test_two_sub_batches_round_trip_and_the_host_form_untouched(bpp, engine, opt):
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    t = 1
    params = _params(bpp, engine, t)
    ms = (PATTERN * 14)[:67]
    d = _data(t, ms, 3)
    ps, cs = _plen(8, t) + 7, 32 * MS
    ref = _host(engine, params, packed, d, ps, cs)
    assert ref["rc"] == 0
    res = None
    for ct, knob in ((0, None), (1, None), (1, "prove_parts"), (1, "prove_fused"), (2, None)):
        opt("ct", ct)
        if knob:
            opt(knob, 0)
        res = _device(engine, params, packed, d, ps, cs)
        _same(engine, res, ref)
        if knob:
            opt(knob, -1)
    again = _host(engine, params, packed, d, ps, cs)  # (the host form before and after device calls on the same context)
    assert np.array_equal(again["proofs"], ref["proofs"]) and np.array_equal(again["commits"], ref["commits"])
    # the outputs verify where they lie: no host copy of a proof or a commitment
    RV = bpp.VerifyAction.RecoverAndVerify
    masks, present = packed.verify_batch_mixed_device(params, res.as_mixed_input(), action=RV)
    for i, m in enumerate(ms):
        assert present[i] == (1 if m == 1 else 0)
        if m == 1:
            assert np.array_equal(masks[i], d["blind"][i, 0]), "recovered mask of item %d is not the blinding factor that went in" % i
    rb = packed.ResidentBatch.from_mixed(params, res.as_mixed_input())
    d2 = _data(t, ms, 33)
    res2 = _device(engine, params, packed, d2, ps, cs)
    assert res2.rc == 0
    filled = rb.refill(res2.as_mixed_input())
    out = rb.enqueue(chunk=16)
    assert filled.result()["code"] == 0
    assert all(r["code"] == 0 for r in out.results())
    rb.close()


# ---------------------------------------------------------------- 4. brought commitments
def test_brought_commitments_and_a_wrong_row(bpp, engine):
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    t = 3
    params = _params(bpp, engine, t)
    d = _data(t, PATTERN * 2, 4)
    ps, cs = _plen(8, t), 32 * MS
    made = _host(engine, params, packed, d, ps, cs)
    assert made["rc"] == 0
    d["commit"] = made["commits"].reshape(len(PATTERN) * 2, MS, 32).copy()
    d["commit"][6, 1] = d["commit"][6, 0]  # item 6 (m = 4): a commitment that is not its opening's
    ref = _host(engine, params, packed, d, ps, cs)
    assert ref["codes"][6] == INVALID_ARGUMENT and ref["texts"][6] == "Witness opening is invalid!"
    res = _device(engine, params, packed, d, ps, cs)
    _same(engine, res, ref)
    assert not res.proofs[6, :int(res.proof_lens[6])].any() and not res.commitments[6, :128].any()
    assert sum(1 for c in res.codes if c) == 1


# ---------------------------------------------------------------- 5. device findings; 9. secrets
def _spoil(d, i, kind):
    m, t = int(d["m"][i]), d["t"]
    if kind == "value":
        d["values"][i, m - 1] = 1 << d["n_bits"]
    elif kind == "minimum":
        d["minp"][i, m // 2] = 1
        d["minv"][i, m // 2] = d["values"][i, m // 2] + 1
    elif kind == "blinding":
        d["blind"][i, m - 1, t - 1] = np.frombuffer(L_ORDER.to_bytes(32, "little"), dtype=np.uint8)
    elif kind == "nonce":
        d["seeds"][i] = 0xFF
        d["seedp"][i] = 1
    elif kind == "nonce_aggregated":
        d["seeds"][i] = 0
        d["seedp"][i] = 1


@pytest.mark.parametrize("kind,text,n_bits", [("value", "Value exceeds bit vector capacity!", 32), ("minimum", "Minimum value is larger than value", 64),
                                              ("blinding", "blinding factor is not canonical", 64), ("nonce", "seed nonce is not canonical", 64),
                                              ("nonce_aggregated", "Mask recovery is not supported with an aggregated statement", 64)])
def test_device_findings(bpp, engine, kind, text, n_bits):
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    t = 3
    params = _params(bpp, engine, t, n_bits)
    ms = (PATTERN * 14)[:67]
    d = _data(t, ms, 5, n_bits=n_bits)
    # item 0, an item in the middle of a wavefront's four, the last item (aggregated ones for the nonce on an aggregated item)
    at = (1, 22, 66) if kind == "nonce_aggregated" else ((0, 25, 65) if kind == "nonce" else (0, 22, 66))
    for i in at:
        _spoil(d, i, kind)
    ps, cs = _plen(8, t, n_bits) + 3, 32 * MS
    ref = _host(engine, params, packed, d, ps, cs)
    assert [i for i in range(67) if ref["codes"][i]] == list(at) and all(ref["texts"][i] == text for i in at)
    before = packed.prove_device_stats(engine)
    res = _device(engine, params, packed, d, ps, cs)
    _same(engine, res, ref)
    assert res.rc == ref["codes"][at[0]] and res.message == text
    for i in at:
        assert not res.proofs[i, :int(res.proof_lens[i])].any() and not res.commitments[i, :32 * ms[i]].any()
    after = packed.prove_device_stats(engine)
    assert after["device_findings"] - before["device_findings"] == 3 and after["calls"] - before["calls"] == 1
    assert after["items"] - before["items"] == 67 and after["host_findings"] == before["host_findings"]
    _no_secrets_left(engine)


def test_every_item_fails_on_the_device(bpp, engine):
    """Codes, messages and lengths are the host form's.  The rows are not compared with it: bpp_prove_openings returns before it
    zeroes anything when NO item passes its host checks (the slots keep what the caller left there), while the device form zeroes a
    failed item's ranges in every call, as include/bpp.h documents for both.  Asserted here: exactly those ranges are zero."""
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    t = 1
    params = _params(bpp, engine, t)
    d = _data(t, PATTERN, 6)
    for i in range(5):
        _spoil(d, i, "blinding")
    ps, cs = _plen(8, t), 32 * MS
    ref = _host(engine, params, packed, d, ps, cs)
    assert all(ref["codes"])
    res = _device(engine, params, packed, d, ps, cs)
    _same(engine, res, ref, rows=False)
    got_p, got_c = res.proofs.cpu().numpy(), res.commitments.cpu().numpy()
    for i, m in enumerate(PATTERN):
        used = int(res.proof_lens[i])
        assert not got_p[i, :used].any() and (got_p[i, used:] == 0xA5).all()
        assert not got_c[i, :32 * m].any() and (got_c[i, 32 * m:] == 0xA5).all()
    _no_secrets_left(engine)


# ---------------------------------------------------------------- 6. host findings
def test_host_findings(bpp, engine):
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    t = 1
    params = _params(bpp, engine, t)
    ms = [1, 3, 4, 0, 2, 16, 8, 1]
    d = _data(t, ms, 7)
    ps, cs = _plen(8, t), 32 * MS
    before = packed.prove_device_stats(engine)
    ref = _host(engine, params, packed, d, ps, cs)
    assert [int(c != 0) for c in ref["codes"]] == [0, 1, 0, 1, 0, 1, 0, 0]
    _same(engine, _device(engine, params, packed, d, ps, cs), ref)
    assert packed.prove_device_stats(engine)["host_findings"] - before["host_findings"] == 3
    # the strides one byte short for the largest item only
    ref = _host(engine, params, packed, d, ps - 1, cs)
    assert ref["texts"][6] == "proof_stride too small" and sum(1 for c in ref["codes"] if c) == 4
    _same(engine, _device(engine, params, packed, d, ps - 1, cs), ref)
    ref = _host(engine, params, packed, d, ps, cs - 1)
    assert ref["texts"][6] == "commit_stride too small" and sum(1 for c in ref["codes"] if c) == 4
    _same(engine, _device(engine, params, packed, d, ps, cs - 1), ref)
    # the rng rows one byte short for the largest item only: a view of the same rows with a shorter stride is not possible, so the
    # array is cut instead
    short = 32 * (_rounds(8) + 3) - 1
    d["rng"] = np.ascontiguousarray(d["rng"][:, :short])
    ref = _host(engine, params, packed, d, ps, cs)
    assert ref["texts"][6] == "not enough external randomness: need (rounds + 3) * 32 bytes" and sum(1 for c in ref["codes"] if c) == 4
    _same(engine, _device(engine, params, packed, d, ps, cs), ref)


# ---------------------------------------------------------------- 8. refusals before any launch
def test_refusals_before_any_launch(bpp, engine, opt):
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    t = 1
    params = _params(bpp, engine, t)
    d = _data(t, PATTERN, 8)
    d["commit"] = np.zeros((5, MS, 32), dtype=np.uint8)
    ps, cs = _plen(8, t), 32 * MS
    _device(engine, params, packed, d, ps, cs)  # (the arena exists from here on)
    before = packed.prove_device_stats(engine)
    host = {k: np.ascontiguousarray(d[k]) for k in ("values", "blind", "commit", "minv", "minp", "seeds", "seedp", "rng")}
    fields = dict(values="values", blind="blindings32", commit="commitments32", minv="min_values", minp="min_present", seeds="seed_nonces32",
                  seedp="seed_present", rng="rng_bytes")
    args = dict(values="values", blind="blindings", commit="commitments", minv="min_values", minp="min_present", seeds="seed_nonces",
                seedp="seed_present", rng="rng_bytes")

    def openings(replace=None, m=None, state=None):
        kw = {args[k]: _dev(d[k]) for k in args}
        if replace:
            kw[args[replace]] = (host[replace].ctypes.data, host[replace].shape)
        return packed.DeviceOpenings(kw.pop("values"), kw.pop("blindings"), d["m"] if m is None else m, label=LABEL, state=state, **kw)

    def refused(inp, needle, **out):
        proofs = out.get("proofs", torch.zeros((5, ps), dtype=torch.uint8, device="cuda"))
        commits = out.get("commits", torch.zeros((5, cs), dtype=torch.uint8, device="cuda"))
        status = out.get("status")
        with pytest.raises(bpp.ProofError) as e:
            packed.prove_openings_device(params, inp, commitments_out=commits, proofs_out=proofs, status_out=status, commit_stride=cs, proof_stride=ps)
        assert e.value.kind == bpp.ProofErrorKind.InvalidArgument and needle in str(e.value), str(e.value)

    for k in fields:
        refused(openings(replace=k), fields[k])
    hp, hc, hs = np.zeros((5, ps), dtype=np.uint8), np.zeros((5, cs), dtype=np.uint8), np.zeros((5, 2), dtype=np.int32)
    refused(openings(), "proofs_out_dev", proofs=(hp.ctypes.data, hp.shape))
    refused(openings(), "commitments_out_dev", commits=(hc.ctypes.data, hc.shape))
    refused(openings(), "status_dev", status=(hs.ctypes.data, hs.shape))
    # m in device memory (the mirror takes host arrays only: the struct's field is pointed at a device copy)
    inp = openings()
    m_dev = torch.from_numpy(d["m"].view(np.int32)).cuda()
    inp.struct.m = m_dev.data_ptr()
    refused(inp, "m must be host memory")
    bad_state = bytearray(_state().strobe.to_bytes())
    bad_state[200] = 166
    refused(openings(state=bytes(bad_state)), "transcript state has pos >= rate")
    opt("prove_check", 1)
    refused(openings(), "prove_check")
    opt("prove_check", -1)
    assert packed.prove_device_stats(engine) == before
    _no_secrets_left(engine)
