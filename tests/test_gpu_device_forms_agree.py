"""GPU tests: the packed and the mixed device forms are one slot geometry (csrc/ingest.h, csrc/refill.h: packed is the mixed form
whose row is arithmetic), so over a UNIFORM batch they must agree -- bpp_batch_upload_packed_device against
bpp_batch_upload_mixed_device on the same device arrays (m_stride = m, proof_lens all equal), and every refill of the one batch
against the same refill of the other.

The two forms are the reference for each other here; the suites of either form hold it to a fresh upload and to the oracle.

The shape: n_bits = 32, m_max = 2, t = 1, 17 items of m = 2.  Seventeen is one more than the 16 items of a 256-lane workgroup and
one more than four full wavefronts of four items, so the partly filled last wavefront and the second workgroup are exercised; m = 2
is the smallest aggregation at which commitment and promise offsets differ from the item index.  Two corpora of that shape are proved
once; B has a non-canonical d1 at slot 16."""
import importlib

import numpy as np
import pytest
import torch

from oracle.pyref import protocol as O
from tests.helpers import LABEL, Prng, sb

pytestmark = pytest.mark.gpu

L_BYTES = np.frombuffer(bytes.fromhex("edd3f55c1a631258d69cf7a2def9de14" + "00" * 15 + "10"), dtype=np.uint8)  # the group order
N, M, BOUNDS = 17, 2, [0, 5, 17]
SLACK = 24  # bytes between the rows of the proofs array: proof_stride > proof_len
D1 = 1      # t = 1: [t] d1 A A1 B r1 s1 (L R)*


@pytest.fixture(scope="module")
def packed():
    return importlib.import_module("bulletproofs-plus_amd.packed")


def _prove(bpp, params, seed):
    rng = Prng(seed)
    trs, sts, ws, exts = [], [], [], []
    commitments = np.zeros((N, M, 32), dtype=np.uint8)
    min_values = np.zeros((N, M), dtype=np.uint64)
    min_present = np.zeros((N, M), dtype=np.uint8)
    for i in range(N):
        vals = [rng.next_u64() % (1 << 32) for _ in range(M)]
        bl = [[sb(O.random_not_zero(rng))] for _ in range(M)]
        mins = [(v // 3 if (i + j) % 3 == 0 else None) for j, v in enumerate(vals)]
        comms = params.commit_many(vals, bl)
        trs.append(bpp.Transcript.new(LABEL))
        sts.append(bpp.RangeStatement.init(params, comms, mins, None))
        ws.append(bpp.RangeWitness.init([bpp.CommitmentOpening.new(vals[j], bl[j]) for j in range(M)]))
        exts.append(rng.fill_bytes(32 * (6 + 3)))  # 6 rounds: n_bits * m = 64
        commitments[i] = np.frombuffer(b"".join(comms), dtype=np.uint8).reshape(M, 32)
        for j, v in enumerate(mins):
            if v is not None:
                min_values[i, j], min_present[i, j] = v, 1
    raw = [g.to_bytes() for g in bpp.RangeProof.prove_batch_mixed(trs, sts, ws, exts)]
    assert len({len(r) for r in raw}) == 1
    proofs = np.zeros((N, len(raw[0]) + SLACK), dtype=np.uint8)
    for i, r in enumerate(raw):
        proofs[i, :len(r)] = np.frombuffer(r, dtype=np.uint8)
    return dict(proofs=proofs, proof_len=len(raw[0]), commitments=commitments, min_values=min_values, min_present=min_present)


@pytest.fixture(scope="module")
def corpora(bpp, engine):
    """(params, A, B, B with a foreign first byte at slot 0): proved once, read-only"""
    params = bpp.RangeParameters.init(32, 2, bpp.create_pedersen_gens_with_extension_degree(1), engine=engine)
    a, b = _prove(bpp, params, b"forms-agree-A"), _prove(bpp, params, b"forms-agree-B")
    assert a["proof_len"] == b["proof_len"] and a["proofs"].tobytes() != b["proofs"].tobytes()
    b["proofs"][16, D1:D1 + 32] = L_BYTES
    foreign = dict(b, proofs=b["proofs"].copy())
    foreign["proofs"][0, 0] = 2
    for d in (a, b, foreign):
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    yield params, a, b, foreign
    params.close()


def _inputs(packed, d):
    """the corpus in device memory ONCE, described as a packed batch and as a mixed batch: the same six addresses"""
    proofs = torch.from_numpy(d["proofs"].copy()).cuda()
    commitments = torch.from_numpy(d["commitments"].copy()).cuda()
    min_values = torch.from_numpy(d["min_values"].view(np.int64).copy()).cuda()
    min_present = torch.from_numpy(d["min_present"].copy()).cuda()
    torch.cuda.synchronize()
    pk = packed.DevicePackedInput(proofs[:, :d["proof_len"]], commitments, min_values, min_present, None, LABEL)
    mx = packed.DeviceMixedInput(proofs, np.full(N, d["proof_len"], dtype=np.uintp), np.full(N, M, dtype=np.uint32), commitments, min_values,
                                 min_present, None, LABEL)
    assert pk.struct.proofs == mx.struct.proofs and pk.struct.proof_stride == mx.struct.proof_stride == d["proof_len"] + SLACK
    assert pk.struct.commitments32 == mx.struct.commitments32 and mx.struct.m_stride == M
    return pk, mx


def _verdicts(bpp, rb):
    """(records, masks, present) of one enqueue over BOUNDS, on the host"""
    e = rb.enqueue(bounds=BOUNDS, actions=[int(bpp.VerifyAction.VerifyOnly), int(bpp.VerifyAction.RecoverAndVerify)])
    e.wait()
    out = [e.verdicts.cpu().numpy().copy()]
    for t in (e.masks, e.present):
        out.append(None if t is None else t.cpu().numpy().copy())
    return out


def _same(got, want, what):
    assert got[0].tolist() == want[0].tolist(), (what, got[0], want[0])
    for g, w in zip(got[1:], want[1:]):
        assert (g is None) == (w is None) and (g is None or g.tobytes() == w.tobytes()), what


@pytest.fixture(scope="module")
def batches(packed, corpora, engine):
    """corpus A resident twice: through the packed and through the mixed device upload, both on their device path"""
    params, a, _, _ = corpora
    pk, mx = _inputs(packed, a)
    before = packed.ingest_stats(engine)
    rb_packed = packed.ResidentBatch(params, pk, None, None, None, None, LABEL, form="device")
    rb_mixed = packed.ResidentBatch.from_mixed(params, mx)
    after = packed.ingest_stats(engine)
    assert after[0] == before[0] + 2 and after[1] == before[1]  # (device_calls, host_fallback_calls)
    yield rb_packed, rb_mixed
    rb_packed.close()
    rb_mixed.close()


def test_uploads_agree(bpp, packed, batches):
    rb_packed, rb_mixed = batches
    got, want = _verdicts(bpp, rb_mixed), _verdicts(bpp, rb_packed)
    _same(got, want, "upload")
    assert (want[0][:, :3] == 0).all() and (want[0][:, 3] == packed.VERDICT_WRITTEN).all(), want[0]  # (a valid corpus: Ok)


FORMS = [("plain", dict()), ("count 9", dict(count=9)), ("mask", dict(live=np.array([1, 0] * 8 + [1], dtype=np.uint8)))]


def test_refills_agree(bpp, packed, corpora, batches):
    """runs behind test_uploads_agree: a refilled batch takes enqueued calls only"""
    _, _, b, foreign = corpora
    rb_packed, rb_mixed = batches
    W, FINDING, FALLBACK = packed.REFILL_WRITTEN, packed.REFILL_FINDING, packed.REFILL_FALLBACK
    # the record's flags per corpus and form: slot 16 (non-canonical d1) is live in the plain and the mask form, dead under the count;
    # the foreign first byte at slot 0 is live in every form and comes before any finding
    expected = {"B": {"plain": W | FINDING, "count 9": W, "mask": W | FINDING}, "foreign": {f: W | FALLBACK for f, _ in FORMS}}
    for name, d in (("B", b), ("foreign", foreign)):
        pk, mx = _inputs(packed, d)
        for form, how in FORMS:
            records, verdicts = [], []
            for rb, inp in ((rb_packed, pk), (rb_mixed, mx)):
                kw = dict(how)
                if "count" in kw:
                    kw["count"] = torch.tensor([kw["count"]], dtype=torch.int32, device="cuda")
                if "live" in kw:
                    kw["live"] = torch.from_numpy(kw["live"].copy()).cuda()
                torch.cuda.synchronize()  # (complete before the engine's stream reads them)
                filled = rb.refill(inp, **kw)
                verdicts.append(_verdicts(bpp, rb))
                filled.wait()
                records.append(filled.record.cpu().numpy().tolist())  # code, msg, index, flags
            assert records[1] == records[0], (name, form, records)
            _same(verdicts[1], verdicts[0], (name, form))
            assert records[0][3] == expected[name][form], (name, form, records[0])
            if records[0][3] & FINDING:
                assert records[0][2] == 16, (name, form, records[0])
