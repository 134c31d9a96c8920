"""GPU tests of the packed form from arrays that already lie in device memory (bpp_batch_upload_packed_device /
bpp_verify_batch_packed_device, csrc/ingest.h): one kernel checks and packs the batch where it lies, nothing passes through the host.
Every expectation is the HOST packed form on the same bytes (tests/test_gpu_packed.py and tests/test_gpu_round3.py hold that form to
the object API and the oracle): resident batches' traces, masks, return codes and message texts.  Proofs come from the engine's batch
prover (bench.make_inputs, as tests/test_gpu_round3.py makes them); the arrays reach the device with torch."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from tests.helpers import LABEL

pytestmark = pytest.mark.gpu

L_BYTES = bytes.fromhex("edd3f55c1a631258d69cf7a2def9de14" + "00" * 15 + "10")  # the group order, little-endian


@pytest.fixture(scope="module")
def packed():
    return importlib.import_module("bulletproofs-plus_amd.packed")


@pytest.fixture(scope="module")
def batches(bpp, packed, engine):
    """(n_bits, m, t, count) -> (params, arrays), made once per module and never changed (tests work on copies)"""
    import bench
    made = {}

    def get(n_bits, m, t, count):
        key = (n_bits, m, t, count)
        if key not in made:
            params = bpp.RangeParameters.init(n_bits, m, bpp.create_pedersen_gens_with_extension_degree(t), engine=engine)
            made[key] = (params, bench.make_inputs(np, packed, params, count, seed=9100 + 7 * n_bits + 3 * m + t))
        return made[key]

    yield get
    for params, _ in made.values():
        params.close()


def _dev(a):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)  # torch's uint64 is thin: the bit patterns travel as int64
    return torch.from_numpy(a).cuda()


def _forms(packed, d, proofs=None, commitments=None, min_values=None, min_present=None, seeds=None, seed_present=None, state=None,
           proof_len=None, label=LABEL):
    """the same bytes as a host PackedInput and as a DevicePackedInput; proof_len overrides the length the structs claim (the rows stay
    where they are: the stride is the arrays')"""
    proofs = d["proofs"] if proofs is None else proofs
    commitments = d["commitments"] if commitments is None else commitments
    min_values = d["min_values"] if min_values is None else min_values
    min_present = d["min_present"] if min_present is None else min_present
    host = packed.PackedInput(proofs, commitments, min_values, min_present, seeds, label, seed_present=seed_present, state=state)
    dev = packed.DevicePackedInput(_dev(proofs), _dev(commitments), _dev(min_values), _dev(min_present), _dev(seeds), label,
                                   seed_present=_dev(seed_present), state=state)
    if proof_len is not None:
        host.struct.proof_len = dev.struct.proof_len = proof_len
    assert dev.struct.proof_stride == host.struct.proof_stride and dev.struct.n_items == host.struct.n_items
    return host, dev


def _call(params, inp, action, chunk, device):
    """one blocking C call -> (return code, errbuf text, masks bytes, presence list)"""
    eng, t = params.engine, int(params.extension_degree())
    masks = np.zeros((inp.n, t, 32), dtype=np.uint8)
    present = np.zeros(inp.n, dtype=np.uint8)
    err = ctypes.create_string_buffer(256)
    if device:
        inp.order_before(eng)
    fn = eng.lib.bpp_verify_batch_packed_device if device else eng.lib.bpp_verify_batch_packed
    rc = fn(eng.ctx, params.handle, ctypes.byref(inp.struct), int(action), chunk, masks.ctypes.data, present.ctypes.data, err, 256)
    return rc, err.value.decode(), masks.tobytes(), present.tolist()


def _same_outcome(params, host, dev, action=0, chunk=0):
    want, got = _call(params, host, action, chunk, False), _call(params, dev, action, chunk, True)
    assert got == want, (got[:2], want[:2])
    return want


# ---- (a) parity of shapes: 1 / 65 / 257 straddle the wavefront and workgroup edges of a kernel with 16 lanes per proof
@pytest.mark.parametrize("n_bits,m,t,count", [(8, 1, 1, 1), (8, 1, 1, 65), (8, 1, 1, 257), (16, 4, 2, 3), (64, 2, 3, 2)])
def test_device_ingest_equals_host_ingest(bpp, packed, batches, n_bits, m, t, count):
    params, d = batches(n_bits, m, t, count)
    seeds = d["seeds"]
    every_other = None if seeds is None else (np.arange(count) % 2 == 0).astype(np.uint8)
    rh = packed.ResidentBatch(params, d["proofs"], d["commitments"], d["min_values"], d["min_present"], seeds, LABEL, seed_present=every_other)
    rd = packed.ResidentBatch(params, _dev(d["proofs"]), _dev(d["commitments"]), _dev(d["min_values"]), _dev(d["min_present"]), _dev(seeds),
                              LABEL, form="device", seed_present=_dev(every_other))
    assert rd.shape() == rh.shape()
    for chunk in (0, 256):
        rh.verify_only(chunk)
        rd.verify_only(chunk)
        for what in (1, 2, 3, 4, 5, 6):
            assert rd.trace(what) == rh.trace(what), (chunk, what)
        assert rd.trace(6) == bytes(32) * rd.shape()["groups"]
    if m == 1:
        for action in (bpp.VerifyAction.RecoverAndVerify, bpp.VerifyAction.RecoverOnly):
            mh, ph = rh.verify_arrays(action, 0)
            md, pd = rd.verify_arrays(action, 0)
            assert pd.tolist() == ph.tolist() == every_other.tolist()
            assert md.tobytes() == mh.tobytes()
            assert md[0].tobytes() == d["blindings"][0, 0].tobytes()  # the blinding the prover was given
    rh.close()
    rd.close()
    # ... and the one-call form
    host, dev = _forms(packed, d, seeds=seeds, seed_present=every_other)
    action = bpp.VerifyAction.RecoverAndVerify if m == 1 else bpp.VerifyAction.VerifyOnly
    rc, _, _, present = _same_outcome(params, host, dev, action, 256)
    assert rc == 0 and present == ([0] * count if m > 1 else every_other.tolist())
    masks, present2 = packed.verify_batch_device(params, dev, action, 256)
    assert present2.tolist() == present


# ---- (b) source layout: rows further apart than their length, in a view that starts 3 bytes into its allocation
def test_strided_unaligned_source(bpp, packed, batches):
    params, d = batches(8, 1, 1, 65)
    count, plen = d["proofs"].shape
    stride = plen + 7
    flat = np.full(3 + count * stride, 0xee, dtype=np.uint8)
    rows = np.lib.stride_tricks.as_strided(flat[3:], shape=(count, plen), strides=(stride, 1))
    rows[:] = d["proofs"]
    base = torch.from_numpy(flat).cuda()
    view = torch.as_strided(base, (count, plen), (stride, 1), 3)
    assert view.data_ptr() == base.data_ptr() + 3 and view.data_ptr() % 4 == 3
    dev = packed.DevicePackedInput(view, _dev(d["commitments"]), _dev(d["min_values"]), _dev(d["min_present"]), _dev(d["seeds"]), LABEL)
    assert dev.struct.proof_stride == stride
    rd = packed.ResidentBatch(params, dev, None, None, None, None, LABEL, form="device")
    rh = packed.ResidentBatch(params, d["proofs"], d["commitments"], d["min_values"], d["min_present"], d["seeds"], LABEL)
    for r in (rd, rh):
        r.verify_arrays(bpp.VerifyAction.RecoverAndVerify, 0)
    for what in (1, 2, 3, 4, 5, 6):
        assert rd.trace(what) == rh.trace(what), what
    assert rd._masks.tobytes() == rh._masks.tobytes() == d["blindings"][:, 0].tobytes()
    rd.close()
    rh.close()
    # the same layout with one proof of another first byte: the staged fall-back brings the rows together
    flat2 = flat.copy()
    flat2[3 + 4 * stride] = 2
    host = packed.PackedInput(np.lib.stride_tricks.as_strided(flat2[3:], shape=(count, plen), strides=(stride, 1)).copy(), d["commitments"],
                              d["min_values"], d["min_present"], None, LABEL)
    base2 = torch.from_numpy(flat2).cuda()
    dev2 = packed.DevicePackedInput(torch.as_strided(base2, (count, plen), (stride, 1), 3), _dev(d["commitments"]), _dev(d["min_values"]),
                                    _dev(d["min_present"]), None, LABEL)
    assert _same_outcome(params, host, dev2)[0] != 0


# ---- (c) findings by class, code and errbuf text against the host form, five proofs each
def _put(proofs, item, offset, value=L_BYTES):
    out = proofs.copy()
    out[item, offset:offset + 32] = np.frombuffer(value, dtype=np.uint8)
    return out


def test_findings_equal_the_host_form(bpp, packed, engine, batches):
    K = bpp.ProofErrorKind
    params, d = batches(8, 1, 1, 5)
    t, plen = 1, d["proofs"].shape[1]
    r1, s1, d1, A = 1 + 32 * (t + 3), 1 + 32 * (t + 4), 1, 1 + 32 * t

    def both(want_rc, want_text, prm=params, chunk=0, data=d, **kw):
        rc, text, _, _ = _same_outcome(prm, *_forms(packed, data, **kw), chunk=chunk)
        assert rc == int(want_rc) and want_text in text, (rc, text)

    both(K.InvalidArgument, "Invalid parsing", proofs=_put(d["proofs"], 3, r1))
    # l in d1[0] of item 1 under a length cut by 32: the length finding is uniform, item 0 reports it
    both(K.InvalidLength, "Unused data after deserialization", proofs=_put(d["proofs"], 1, d1), proof_len=plen - 32)
    sevens = d["proofs"].copy()
    sevens[:, 0] = 7
    both(K.InvalidArgument, "Extension degree not valid", proofs=sevens)
    both(K.InvalidLength, "Serialized proof is too short", proof_len=1 + 32 * (t + 5))
    both(K.InvalidLength, "Unused data after deserialization", proof_len=plen - 1)
    bad_state = bytes(200) + bytes([166, 0, 0])  # pos >= rate
    both(K.InvalidArgument, "transcript state has pos >= rate", state=bad_state)
    both(K.InvalidArgument, "Invalid parsing", state=bad_state, proofs=_put(d["proofs"], 0, r1))
    # one bit flipped in A.  Whether the flipped bytes still decode to a point depends on the bit; the host form (the reference here)
    # says which of the first bits gives the class this case is about
    for bit in range(16):
        flipped = d["proofs"].copy()
        flipped[2, A + 5 + bit // 8] ^= 1 << (bit % 8)
        if _call(params, _forms(packed, d, proofs=flipped)[0], 0, 0, False)[0] == int(K.VerificationFailed):
            break
    else:
        raise AssertionError("no bit flip in A that the host form answers with VerificationFailed")
    both(K.VerificationFailed, "", proofs=flipped)
    # l in s1 of item 2, a nonce with m = 2 only at item 3: index 2 wins
    params2, d2 = batches(8, 2, 1, 5)
    nonces = np.random.default_rng(5).integers(1, 256, size=(5, 32), dtype=np.uint8)
    only3 = np.array([0, 0, 0, 1, 0], dtype=np.uint8)
    both(K.InvalidArgument, "Invalid parsing", prm=params2, data=d2, proofs=_put(d2["proofs"], 2, s1), seeds=nonces, seed_present=only3)
    both(K.InvalidArgument, "Mask recovery is not supported with an aggregated statement", prm=params2, data=d2, seeds=nonces,
         seed_present=only3)
    # m = 2 proofs offered under m = 1 statements: recorded at upload, raised at verify time
    both(K.InvalidLength, "Vector L/R length not adequate", prm=params2, data=d2, commitments=d2["commitments"][:, :1].copy(),
         min_values=d2["min_values"][:, :1].copy(), min_present=d2["min_present"][:, :1].copy())
    # parameters of t = 2 over t = 1 proofs, a promise of 2^16 at n = 16 in an earlier item: the degree finding comes first
    params16, d16 = batches(16, 1, 1, 5)
    p16t2 = bpp.RangeParameters.init(16, 1, bpp.create_pedersen_gens_with_extension_degree(2), engine=engine)
    mins = d16["min_values"].copy()
    mins[1, 0] = 1 << 16
    for chunk in (0, 2):
        both(K.InvalidArgument, "Inconsistent extension degree", prm=p16t2, data=d16, min_values=mins, chunk=chunk)
    both(K.InvalidLength, "Minimum value promise exceeds bit vector capacity", prm=params16, data=d16, min_values=mins)
    p16t2.close()


# ---- (d) mixed first bytes: the staged fall-back, counted; (f) nothing secret is left behind by either path
def _secret_bytes(eng, handle=0):
    n = ctypes.c_uint64()
    assert eng.lib.bpp_batch_secret_bytes(eng.ctx, handle, ctypes.byref(n)) == 0
    return n.value


def test_mixed_first_bytes_take_the_host_path(bpp, packed, engine, batches):
    params, d = batches(8, 1, 1, 5)
    mixed = d["proofs"].copy()
    mixed[3, 0] = 2
    host, dev = _forms(packed, d, proofs=mixed, seeds=d["seeds"])
    before = packed.ingest_stats(engine)
    rc, text, _, _ = _same_outcome(params, host, dev, bpp.VerifyAction.RecoverOnly)
    assert rc != 0 and text
    after = packed.ingest_stats(engine)
    assert (after[0], after[1]) == (before[0], before[1] + 1) and after[2] > before[2]
    assert _secret_bytes(engine) == 0
    host, dev = _forms(packed, d, seeds=d["seeds"])
    rc, _, masks, present = _same_outcome(params, host, dev, bpp.VerifyAction.RecoverOnly)
    assert rc == 0 and present == [1] * 5 and masks == d["blindings"][:, 0].tobytes()
    clean = packed.ingest_stats(engine)
    assert (clean[0], clean[1]) == (after[0] + 1, after[1])


def test_secrets_are_wiped_with_the_batch(bpp, packed, engine, batches):
    params, d = batches(8, 1, 1, 65)
    rd = packed.ResidentBatch(params, _dev(d["proofs"]), _dev(d["commitments"]), _dev(d["min_values"]), _dev(d["min_present"]),
                              _dev(d["seeds"]), LABEL, form="device")
    assert _secret_bytes(engine, rd.handle) > 65 * 24  # the nonces arrived
    masks, present = rd.verify_arrays(bpp.VerifyAction.RecoverOnly, 0)
    assert present.tolist() == [1] * 65 and masks.tobytes() == d["blindings"][:, 0].tobytes()
    assert _secret_bytes(engine, rd.handle) > 2 * 65 * 24  # nonces + masks
    rd.close()
    assert _secret_bytes(engine) == 0  # what the next upload adopts holds nothing


# ---- (e) pointer kinds, through bpp_device_pointer_check only: nothing is launched.  (No host address is handed to the two ingest
# calls here; upload_device_form in csrc/engine.hip runs every non-null array through the same check before it allocates or
# launches anything.)
def test_pointer_kinds(packed, engine):
    t = torch.zeros(64, dtype=torch.uint8, device="cuda")
    assert packed.device_pointer_kind(engine, t.data_ptr()) == 0
    assert packed.device_pointer_kind(engine, t.data_ptr() + 17) == 0
    a = np.zeros(64, dtype=np.uint8)
    assert packed.device_pointer_kind(engine, a.ctypes.data) == 2
    torch.cuda.synchronize()  # the query left no runtime error behind: the next runtime call is clean
    with pytest.raises(Exception):
        packed.DevicePackedInput(torch.zeros((2, 65), dtype=torch.uint8), t.view(2, 1, 32))  # a host tensor is refused by the wrapper


# ---- (g) stream ordering: an engine on torch's current stream, inputs produced on that stream, no synchronisation in between
def test_engine_on_the_producers_stream(bpp, packed, batches):
    _, d = batches(8, 1, 1, 65)
    src = [_dev(d[k]) for k in ("proofs", "commitments", "min_values", "min_present", "seeds")]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        eng = bpp.Engine(0, stream=stream.cuda_stream)
        params = bpp.RangeParameters.init(8, 1, bpp.create_pedersen_gens_with_extension_degree(1), engine=eng)
        made = [x.clone() for x in src]  # device-side copies on `stream`, still in flight when the engine is called
        inp = packed.DevicePackedInput(*made, LABEL)
        masks, present = packed.verify_batch_device(params, inp, bpp.VerifyAction.RecoverAndVerify, 0)
        assert inp.synchronised is False
        assert present.tolist() == [1] * 65 and masks.tobytes() == d["blindings"][:, 0].tobytes()
        # on any other stream the wrapper orders by synchronising
        other = bpp.Engine(0)
        p2 = bpp.RangeParameters.init(8, 1, bpp.create_pedersen_gens_with_extension_degree(1), engine=other)
        inp2 = packed.DevicePackedInput(*[x.clone() for x in src], LABEL)
        packed.verify_batch_device(p2, inp2, bpp.VerifyAction.VerifyOnly, 0)
        assert inp2.synchronised is True
        p2.close()
        other.close()
        params.close()
        eng.close()
