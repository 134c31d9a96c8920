"""GPU tests of the array form for batches of mixed aggregation factors (bpp_batch_upload_mixed / bpp_verify_batch_mixed and their
_device forms, csrc/ingest.h with the host side in csrc/ingest_mixed.h): rows of proof_stride bytes and m_stride entries, the used
part of every row in two host arrays.
Every expectation is the ITEM form (bpp_batch_upload / bpp_verify_batch) on a bpp_verify_item array that points into the same rows:
the batch's shape, every trace, return codes, message texts, masks and presence.  Proofs come from bpp_prove_batch_mixed
(tests/test_gpu_prove_mixed.py holds it to the oracle); the arrays reach the device with torch.

The C ABI reports a construction finding as {code, text}; which ITEM it names shows in which of two planted findings wins (the lower
index).  The index itself is compared where the ABI hands it out (the deferred tiers, bpp_verify_resident_groups) and, for the
construction tier, by the host harness (tests/test_ingest_mixed_host.py)."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from oracle import cport
from oracle.pyref import protocol as O
from tests.helpers import LABEL, Prng, sb

pytestmark = pytest.mark.gpu

L_BYTES = np.frombuffer(bytes.fromhex("edd3f55c1a631258d69cf7a2def9de14" + "00" * 15 + "10"), dtype=np.uint8)  # the group order
PATTERN = [4, 1, 2, 1, 1, 4, 2]
M_STRIDE = 8
SLACK = 40  # bytes between the longest proof and the row stride of the plain rows


@pytest.fixture(scope="module")
def packed():
    return importlib.import_module("bulletproofs-plus_amd.packed")


@pytest.fixture(scope="module")
def made(bpp, engine):
    """(n_bits, m_max, t) -> (params, rows of 67 items in the m pattern), proved once per module by ONE bpp_prove_batch_mixed call and
    never changed (tests work on copies).  Nonces on the m = 1 items, promises on every third opening."""
    cache = {}

    def get(n_bits, m_max, t, count=67):
        key = (n_bits, m_max, t)
        if key in cache:
            return cache[key]
        params = bpp.RangeParameters.init(n_bits, m_max, bpp.create_pedersen_gens_with_extension_degree(t), engine=engine)
        rng = Prng(b"mixed-inputs-%d-%d-%d" % key)
        ms = [min(PATTERN[i % 7], m_max) for i in range(count)]
        trs, sts, ws, exts, blinds = [], [], [], [], []
        commitments = np.full((count, M_STRIDE, 32), 0, dtype=np.uint8)
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
        got = bpp.RangeProof.prove_batch_mixed(trs, sts, ws, exts)
        raw = [g.to_bytes() for g in got]
        lens = np.array([len(r) for r in raw], dtype=np.uintp)
        proofs = np.zeros((count, int(lens.max()) + SLACK), dtype=np.uint8)
        for i, r in enumerate(raw):
            proofs[i, :len(r)] = np.frombuffer(r, dtype=np.uint8)
        d = dict(proofs=proofs, lens=lens, m=np.array(ms, dtype=np.uint32), commitments=commitments, min_values=min_values,
                 min_present=min_present, seeds=seeds, seed_present=(np.array(ms) == 1).astype(np.uint8), blinds=blinds)
        cache[key] = (params, d)
        return cache[key]

    yield get
    for params, _ in cache.values():
        params.close()


def _pick(d, idx):
    """the rows of the items `idx` (a count: the first so many), copied"""
    idx = list(range(idx)) if isinstance(idx, int) else list(idx)
    out = {k: (v[idx].copy() if isinstance(v, np.ndarray) else [v[i] for i in idx]) for k, v in d.items()}
    return out


def _dev(a):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)  # torch's uint64 is thin: the bit patterns travel as int64
    return torch.from_numpy(a).cuda()


def _rows(a):
    return a.ctypes.data + np.arange(a.shape[0], dtype=np.uint64) * np.uint64(a.strides[0])


class _Batch:
    """one upload: .rc, .text and, when it succeeded, .rb (a packed.ResidentBatch)"""

    def __init__(self, packed, params, form, d, nonces, state=None):
        eng = params.engine
        self.keep, self.rb = [d], None
        seeds = d["seeds"] if nonces else None
        seed_present = d["seed_present"] if nonces else None
        handle = ctypes.c_uint64()
        err = ctypes.create_string_buffer(256)
        n = d["proofs"].shape[0]
        if form == "items":
            lbl = np.frombuffer(LABEL, dtype=np.uint8).copy()
            items = np.zeros(n, dtype=packed._VERIFY_ITEM)
            items["proof"] = _rows(d["proofs"])
            items["proof_len"] = d["lens"]
            items["commitments32"] = _rows(d["commitments"])
            items["m"] = d["m"]
            items["min_values"] = _rows(d["min_values"])
            items["min_present"] = _rows(d["min_present"])
            if nonces:
                items["seed_nonce32"] = np.where(seed_present != 0, _rows(seeds), np.uint64(0))
            if state is not None:
                st = np.frombuffer(bytes(state), dtype=np.uint8).copy()
                self.keep.append(st)
                items["transcript_state"] = st.ctypes.data
            items["transcript_label"] = lbl.ctypes.data
            items["label_len"] = len(LABEL)
            self.keep += [items, lbl]
            lib = importlib.import_module("bulletproofs-plus_amd._lib")
            self.rc = eng.lib.bpp_batch_upload(eng.ctx, params.handle, items.ctypes.data_as(ctypes.POINTER(lib.VerifyItem)), n,
                                               ctypes.byref(handle), err, 256)
        else:
            if form == "host":
                inp = packed.MixedInput(d["proofs"], d["lens"], d["m"], d["commitments"], d["min_values"], d["min_present"], seeds, LABEL,
                                        seed_present=seed_present, state=state)
                fn = eng.lib.bpp_batch_upload_mixed
            else:
                proofs = d["proofs_dev"] if "proofs_dev" in d else _dev(d["proofs"])
                inp = packed.DeviceMixedInput(proofs, d["lens"], d["m"], _dev(d["commitments"]), _dev(d["min_values"]), _dev(d["min_present"]),
                                              _dev(seeds), LABEL, seed_present=_dev(seed_present), state=state)
                inp.order_before(eng)
                fn = eng.lib.bpp_batch_upload_mixed_device
            self.keep.append(inp)
            self.inp = inp
            self.rc = fn(eng.ctx, params.handle, ctypes.byref(inp.struct), ctypes.byref(handle), err, 256)
        self.text = err.value.decode()
        if self.rc == 0:
            rb = packed.ResidentBatch.__new__(packed.ResidentBatch)
            rb.params, rb.engine, rb.t, rb.n, rb.handle = params, eng, int(params.extension_degree()), n, handle
            self.rb = rb

    def verify(self, action, chunk):
        """bpp_verify_resident -> (rc, text, masks bytes, presence list)"""
        rb = self.rb
        masks = np.zeros((rb.n, rb.t, 32), dtype=np.uint8)
        present = np.zeros(rb.n, dtype=np.uint8)
        err = ctypes.create_string_buffer(256)
        rc = rb.engine.lib.bpp_verify_resident(rb.engine.ctx, rb.handle, int(action), chunk, masks.ctypes.data, present.ctypes.data, err, 256)
        return rc, err.value.decode(), masks.tobytes(), present.tolist()

    def traces(self):
        out = []
        for what in range(1, 9):
            try:
                out.append(self.rb.trace(what))
            except Exception as e:  # (a kind the last verification did not produce: the refusal is compared)
                out.append(("refused", str(e)))
        return out

    def close(self):
        if self.rb is not None:
            self.rb.close()


FORMS = ("items", "host", "device")


def _three(packed, params, d, nonces, state=None, dev=None):
    """the same rows through the item form, the mixed host form and the mixed device form; `dev`: other rows for the two mixed
    forms (same used bytes, another geometry)"""
    return [_Batch(packed, params, form, d if (form == "items" or dev is None) else dev, nonces, state) for form in FORMS]


def _same_everywhere(bpp, batches, nonces, chunks=(0, 4)):
    """shape, verification outcomes and traces of the three batches are equal; returns the item form's outcomes"""
    ref = batches[0]
    assert all(b.rc == 0 for b in batches), [(b.rc, b.text) for b in batches]
    for b in batches[1:]:
        assert b.rb.shape() == ref.rb.shape()
    actions = [bpp.VerifyAction.RecoverAndVerify] if nonces else [bpp.VerifyAction.VerifyOnly]
    seen = []
    for chunk in chunks:
        for action in actions:
            want = ref.verify(action, chunk)
            want_traces = ref.traces()
            for form, b in zip(FORMS[1:], batches[1:]):
                assert b.verify(action, chunk) == want, (form, chunk, action, want[:2])
                got = b.traces()
                for what, (g, w) in enumerate(zip(got, want_traces), 1):
                    assert g == w, (form, chunk, what)
            seen.append(want)
    return seen


# ---- 1. equals the item form
@pytest.mark.parametrize("n_bits,m_max,t,n_items", [(8, 4, 1, 1), (8, 4, 1, 5), (8, 4, 1, 17), (8, 4, 1, 67), (8, 4, 2, 1), (8, 4, 2, 5),
                                                    (8, 4, 2, 17), (8, 4, 2, 67), (64, 2, 3, 5)])
def test_mixed_forms_equal_the_item_form(bpp, packed, made, n_bits, m_max, t, n_items):
    params, full = made(n_bits, m_max, t, 67 if n_bits == 8 else 5)
    d = _pick(full, n_items)
    for nonces in (False, True):
        batches = _three(packed, params, d, nonces)
        for rc, text, masks, present in _same_everywhere(bpp, batches, nonces):
            assert rc == 0, text
            if nonces:
                assert present == d["seed_present"].tolist()
                m = np.frombuffer(masks, dtype=np.uint8).reshape(n_items, t * 32)
                for i in range(n_items):
                    if present[i]:
                        assert m[i].tobytes() == d["blinds"][i]  # the blinding the prover was given
        for b in batches:
            b.close()
    # the one-call forms
    host = packed.MixedInput(d["proofs"], d["lens"], d["m"], d["commitments"], d["min_values"], d["min_present"], d["seeds"], LABEL,
                             seed_present=d["seed_present"])
    dev = packed.DeviceMixedInput(_dev(d["proofs"]), d["lens"], d["m"], _dev(d["commitments"]), _dev(d["min_values"]), _dev(d["min_present"]),
                                  _dev(d["seeds"]), LABEL, seed_present=_dev(d["seed_present"]))
    mh, ph = packed.verify_batch_mixed(params, host, bpp.VerifyAction.RecoverAndVerify, 4)
    md, pd = packed.verify_batch_mixed_device(params, dev, bpp.VerifyAction.RecoverAndVerify, 4)
    assert pd.tolist() == ph.tolist() == d["seed_present"].tolist() and md.tobytes() == mh.tobytes()
    rb = packed.ResidentBatch.from_mixed(params, dev)
    masks, present = rb.verify_arrays(bpp.VerifyAction.RecoverAndVerify, 0)
    assert present.tolist() == ph.tolist() and masks.tobytes() == mh.tobytes()
    rb.close()


def test_verdicts_equal_the_oracle(bpp, packed, made):
    """one valid batch and one with a single flipped bit in an L: the three forms agree with each other and with oracle.cport"""
    n_bits, m_max, t = 8, 4, 1
    params, full = made(n_bits, m_max, t)
    cp = cport.Params(n_bits, m_max, t)
    for flip in (False, True):
        d = _pick(full, 5)
        if flip:
            d["proofs"][2, 1 + 32 * (t + 5) + 3] ^= 0x10  # L_0 of item 2
        batch = [dict(proof=d["proofs"][i, :int(d["lens"][i])].tobytes(),
                      commitments=[d["commitments"][i, j].tobytes() for j in range(int(d["m"][i]))],
                      min_values=[int(d["min_values"][i, j]) if d["min_present"][i, j] else None for j in range(int(d["m"][i]))],
                      seed_nonce=None, label=LABEL) for i in range(5)]
        want_rc = cp.verify(batch, 0)[0]
        assert (want_rc != 0) == flip
        batches = _three(packed, params, d, False)
        for rc, _text, _m, _p in _same_everywhere(bpp, batches, False):
            assert rc == want_rc
        for b in batches:
            b.close()
    cp.close()


# ---- 2. geometry: an odd base, proof_stride = longest + 3, m_stride wider than m_max, every slack byte poisoned
def test_poisoned_slack_and_odd_geometry(bpp, packed, made):
    params, full = made(8, 4, 1)
    d = _pick(full, 17)
    n, longest = 17, int(d["lens"].max())
    stride = longest + 3
    flat = np.full(5 + n * stride, 0xFF, dtype=np.uint8)
    rows = np.lib.stride_tricks.as_strided(flat[5:], shape=(n, longest), strides=(stride, 1))
    for i in range(n):
        rows[i, :int(d["lens"][i])] = d["proofs"][i, :int(d["lens"][i])]
    base = torch.from_numpy(flat).cuda()
    view = torch.as_strided(base, (n, longest), (stride, 1), 5)
    assert view.data_ptr() % 2 == 1
    p = dict(d, proofs=rows, proofs_dev=view)
    p["commitments"], p["min_values"], p["min_present"] = d["commitments"].copy(), d["min_values"].copy(), d["min_present"].copy()
    for i in range(n):
        m = int(d["m"][i])
        p["commitments"][i, m:] = 0xFF
        p["min_values"][i, m:] = 1 << 63
        p["min_present"][i, m:] = 1
    for nonces in (False, True):
        batches = _three(packed, params, d, nonces, dev=p)
        assert batches[1].inp.struct.proof_stride == batches[2].inp.struct.proof_stride == stride and batches[2].inp.struct.m_stride == M_STRIDE
        for rc, text, _m, present in _same_everywhere(bpp, batches, nonces):
            assert rc == 0, text
        for b in batches:
            b.close()


# ---- 3. findings equal the item form's
def _outcome(bpp, packed, params, d, nonces, form):
    """upload and, if that succeeds, one grouped verification: (rc, text) or ("verify", code, tier, index, text)"""
    b = _Batch(packed, params, form, d, nonces)
    try:
        if b.rc != 0:
            return (b.rc, b.text)
        r = packed.verify_groups(b.rb, [0, b.rb.n])[0]
        return ("verify", r["code"], r["tier"], r["index"], r["msg"])
    finally:
        b.close()


def _all_forms(bpp, packed, params, d, nonces=False):
    got = [_outcome(bpp, packed, params, d, nonces, form) for form in FORMS]
    assert got[1] == got[0] and got[2] == got[0], got
    return got[0]


def test_findings_equal_the_item_form(bpp, packed, engine, made):
    K = bpp.ProofErrorKind
    params, full = made(8, 4, 1)
    t = 1
    d1, s1 = 1, 1 + 32 * (t + 4)

    def case(mutate, idx=7, nonces=False):
        d = _pick(full, idx)
        mutate(d)
        return _all_forms(bpp, packed, params, d, nonces)

    def put(item, offset):
        def f(d):
            d["proofs"][item, offset:offset + 32] = L_BYTES
        return f

    def setv(key, item, value):
        def f(d):
            d[key][item] = value
        return f

    def both(*fs):
        def f(d):
            for g in fs:
                g(d)
        return f

    assert case(lambda d: None)[:2] == ("verify", 0)
    assert case(put(3, d1)) == (int(K.InvalidArgument), "Invalid parsing")
    assert case(lambda d: d["lens"].__setitem__(3, d["lens"][3] - 1)) == (int(K.InvalidLength), "Unused data after deserialization")
    assert case(lambda d: d["lens"].__setitem__(3, d["lens"][3] + 32)) == (int(K.InvalidLength), "Unused data after deserialization")
    before = packed.ingest_stats(engine)
    assert case(setv("proofs", (3, 0), 0)) == (int(K.InvalidArgument), "Extension degree not valid")
    assert packed.ingest_stats(engine)[1] == before[1] + 1  # (the first bytes differ: the device form staged it)
    # a nonce on an m = 2 item at index 3 (items 2 and 3 of the pattern change places)
    swapped = [0, 1, 3, 2, 4, 5, 6]
    assert case(setv("seed_present", 3, 1), idx=swapped, nonces=True) == (int(K.InvalidArgument), "Mask recovery is not supported with an aggregated statement")
    # a promise above the capacity: recorded at upload, raised when the item's group is verified, with its index
    r = case(both(setv("min_values", (3, 0), 256), setv("min_present", (3, 0), 1)))
    assert r[:4] == ("verify", int(K.InvalidLength), 3, 3) and "Minimum value promise exceeds bit vector capacity" in r[4]
    assert case(setv("m", 3, 3)) == (int(K.InvalidArgument), "Number of commitments must be a power of two")
    assert case(setv("m", 3, 8)) == (int(K.InvalidArgument), "Not enough generators for this statement")
    # two findings, one the host knows from m[] and one only the kernel finds, in both orders: the lower index wins
    assert case(both(put(1, s1), setv("m", 4, 3))) == (int(K.InvalidArgument), "Invalid parsing")
    assert case(both(setv("m", 1, 8), put(4, s1))) == (int(K.InvalidArgument), "Not enough generators for this statement")
    assert case(both(setv("m", 2, 3), setv("m", 5, 8))) == (int(K.InvalidArgument), "Number of commitments must be a power of two")
    assert case(both(put(2, d1), lambda d: d["lens"].__setitem__(5, d["lens"][5] - 1))) == (int(K.InvalidArgument), "Invalid parsing")
    # the transcript state of the call unusable: item 0's finding once its proof has parsed
    bad_state = bytes(200) + bytes([166, 0, 0])
    got = []
    for form in FORMS:
        b = _Batch(packed, params, form, _pick(full, 7), False, state=bad_state)
        got.append((b.rc, b.text))
        b.close()
    assert got == [(int(K.InvalidArgument), "transcript state has pos >= rate")] * 3


# ---- 4. mixed first bytes: the staged host path, counted, nothing secret left
def _secret_bytes(eng, handle=0):
    n = ctypes.c_uint64()
    assert eng.lib.bpp_batch_secret_bytes(eng.ctx, handle, ctypes.byref(n)) == 0
    return n.value


def test_mixed_first_bytes_take_the_host_path(bpp, packed, engine, made):
    params, full = made(8, 4, 1)
    params2, full2 = made(8, 4, 2)
    d = _pick(full, 7)
    other = _pick(full2, 7)
    # item 3 (m = 1) is a proof of extension degree 2: longer by 32 bytes, another first byte
    d["lens"][3] = other["lens"][3]
    d["proofs"][3] = 0
    d["proofs"][3, :int(other["lens"][3])] = other["proofs"][3, :int(other["lens"][3])]
    before = packed.ingest_stats(engine)
    batches = _three(packed, params, d, True)
    after = packed.ingest_stats(engine)
    assert (after[0], after[1]) == (before[0], before[1] + 1) and after[2] > before[2]
    assert [b.rc for b in batches] == [0, 0, 0]
    for b in batches[1:]:
        assert b.rb.shape() == batches[0].rb.shape()
    want = batches[0].verify(bpp.VerifyAction.RecoverAndVerify, 0)
    assert want[0] == int(bpp.ProofErrorKind.InvalidArgument) and "Inconsistent extension degree" in want[1]
    for b in batches[1:]:
        assert b.verify(bpp.VerifyAction.RecoverAndVerify, 0) == want
    for b in batches:
        b.close()
    assert _secret_bytes(engine) == 0
    # the clean rows take the device path, and the nonces arrive
    clean = _Batch(packed, params, "device", _pick(full, 7), True)
    assert clean.rc == 0 and packed.ingest_stats(engine)[:2] == (after[0] + 1, after[1])
    assert _secret_bytes(engine, clean.rb.handle) > 2 * 24  # three m = 1 items of the seven have a nonce
    rc, _text, _masks, present = clean.verify(bpp.VerifyAction.RecoverOnly, 0)
    assert rc == 0 and present == _pick(full, 7)["seed_present"].tolist()
    clean.close()
    assert _secret_bytes(engine) == 0


# ---- 5. refusals before any launch, each names the field
def test_refusals_name_the_field(bpp, packed, engine, made):
    params, full = made(8, 4, 1)
    d = _pick(full, 5)
    lib = engine.lib

    def upload(inp, device=True):
        handle = ctypes.c_uint64()
        err = ctypes.create_string_buffer(256)
        fn = lib.bpp_batch_upload_mixed_device if device else lib.bpp_batch_upload_mixed
        rc = fn(engine.ctx, params.handle, ctypes.byref(inp.struct), ctypes.byref(handle), err, 256)
        assert handle.value == 0
        return rc, err.value.decode()

    def device_input():
        return packed.DeviceMixedInput(_dev(d["proofs"]), d["lens"], d["m"], _dev(d["commitments"]), _dev(d["min_values"]), _dev(d["min_present"]),
                                       None, LABEL)

    bad = int(bpp.ProofErrorKind.InvalidArgument)
    before = packed.ingest_stats(engine)
    inp = device_input()
    inp.struct.commitments32 = d["commitments"].ctypes.data  # a device array given as a host pointer
    rc, text = upload(inp)
    assert rc == bad and text.startswith("commitments32 is not device memory")
    inp = device_input()
    m_dev = torch.from_numpy(d["m"].view(np.int32)).cuda()
    inp.struct.m = m_dev.data_ptr()  # m given as a device pointer
    rc, text = upload(inp)
    assert rc == bad and text.startswith("m is device memory")
    inp = device_input()
    lens_dev = torch.from_numpy(d["lens"].view(np.int64)).cuda()
    inp.struct.proof_lens = lens_dev.data_ptr()
    rc, text = upload(inp)
    assert rc == bad and text.startswith("proof_lens is device memory")
    host = packed.MixedInput(d["proofs"], d["lens"], d["m"], d["commitments"], d["min_values"], d["min_present"], None, LABEL)
    for device, make in ((True, device_input), (False, lambda: host)):
        inp = make()
        keep = inp.struct.proof_stride
        inp.struct.proof_stride = int(d["lens"].max()) - 1
        rc, text = upload(inp, device)
        assert rc == bad and text == "proof_stride is below a proof length"
        inp.struct.proof_stride = keep
        inp.struct.m_stride = 2
        rc, text = upload(inp, device)
        assert rc == bad and text == "m_stride is below an aggregation factor"
        inp.struct.m_stride = M_STRIDE
    assert packed.ingest_stats(engine) == before  # nothing ran, nothing was staged
    torch.cuda.synchronize()  # ... and the pointer queries left no runtime error behind


# ---- 6. from the prover, no repacking
def test_prover_output_feeds_the_mixed_forms(bpp, packed, engine, made):
    params, _ = made(8, 4, 1)
    n_bits, t, ms = 8, 1, PATTERN
    rng = Prng(b"mixed-inputs-openings")
    trs, ws, mins, nonces, exts = [], [], [], [], []
    for m in ms:
        vals = [rng.next_u64() % (1 << n_bits) for _ in range(m)]
        ws.append(bpp.RangeWitness.init([bpp.CommitmentOpening.new(v, [sb(O.random_not_zero(rng)) for _ in range(t)]) for v in vals]))
        mins.append([None] * m)
        nonces.append(None)
        trs.append(bpp.Transcript.new(LABEL))
        exts.append(rng.fill_bytes(32 * ((n_bits * m).bit_length() - 1 + 3)))
    _p, items, n, _keep = bpp.RangeProof._openings_marshal(trs, ws, mins, nonces, exts, params)
    stride = 1 + 32 * (t + 5 + 2 * 5) + 7
    proofs = np.full((n, stride), 0xEE, dtype=np.uint8)
    comms = np.full((n, M_STRIDE, 32), 0xEE, dtype=np.uint8)
    lens = np.zeros(n, dtype=np.uintp)
    status = (ctypes.c_int * n)()
    err = ctypes.create_string_buffer(256)
    rc = engine.lib.bpp_prove_openings(engine.ctx, params.handle, items, n, comms.ctypes.data, 32 * M_STRIDE, proofs.ctypes.data, stride,
                                       lens.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t)), status, err, 256)
    assert rc == 0 and list(status) == [0] * n, err.value
    m_arr = np.array(ms, dtype=np.uint32)
    host = packed.MixedInput(proofs, lens, m_arr, comms, None, None, None, LABEL)
    assert host.struct.proof_stride == stride and host.struct.m_stride == M_STRIDE
    packed.verify_batch_mixed(params, host, bpp.VerifyAction.VerifyOnly, 0)  # raises unless Ok
    dev = packed.DeviceMixedInput(_dev(proofs), lens, m_arr, _dev(comms), None, None, None, LABEL)
    before = packed.ingest_stats(engine)
    packed.verify_batch_mixed_device(params, dev, bpp.VerifyAction.VerifyOnly, 0)
    assert packed.ingest_stats(engine)[:2] == (before[0] + 1, before[1])


# ---- 7. on the stream
def test_device_made_batch_on_the_stream(bpp, packed, made):
    params, full = made(8, 4, 1)
    d = _pick(full, 17)
    d["proofs"][9, 1 + 32 * 6 + 3] ^= 0x10  # L_0 of item 9: the second group fails, the first does not
    ref = _Batch(packed, params, "items", d, False)
    dev = _Batch(packed, params, "device", d, False)
    assert ref.rc == 0 and dev.rc == 0
    bounds = [0, 5, 17]
    want = packed.verify_groups(ref.rb, bounds)
    assert want[0]["code"] == 0 and want[1]["code"] != 0
    got = dev.rb.enqueue(bounds=bounds).results()
    assert got == want
    # a refill of such a batch is not built: the existing refusal for a batch of another origin
    packed_inp = packed.DevicePackedInput(_dev(d["proofs"][:, :100]), _dev(d["commitments"][:, :1].copy()))
    with pytest.raises(bpp.ProofError) as e:
        dev.rb.refill(packed_inp)
    assert "the batch cannot be refilled: only a batch that bpp_batch_upload_packed_device packed on the device records its shape" in str(e.value)
    ref.close()
    dev.close()
