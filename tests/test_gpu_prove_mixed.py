"""GPU parity tests for the mixed-aggregation prover (bpp_prove_batch_mixed): shuffled batches of every power-of-two
aggregation factor up to m_max give the oracle's bytes under every prover knob, the same bytes as one bpp_prove_batch per
class, per-item errors equal to those of a one-item bpp_prove_batch, and proofs that verify as one mixed batch."""
import ctypes
import random

import pytest

from oracle import cport
from oracle.pyref import curve as C
from oracle.pyref import merlin as M
from oracle.pyref import protocol as O
from tests.helpers import LABEL, Prng, sb

pytestmark = pytest.mark.gpu


def _items(bpp, params, n, t, ms, seed, state=None):
    """one (transcript, statement, witness, rng bytes) per entry of `ms`: seed nonces on every other m = 1 item, minimum-value
    promises on every third opening; the transcript is Transcript::new(LABEL) or, for the items with state[i], `state`"""
    rng = Prng(seed)
    out = []
    for i, m in enumerate(ms):
        rounds = (n * m).bit_length() - 1
        vals = [rng.next_u64() % (1 << min(n, 63)) for _ in range(m)]
        blinds = [[sb(O.random_not_zero(rng)) for _ in range(t)] for _ in range(m)]
        mins = [(v // 3 if (i + j) % 3 == 0 else None) for j, v in enumerate(vals)]
        snonce = sb(O.random_not_zero(rng)) if m == 1 and i % 2 == 0 else None
        ext = rng.fill_bytes(32 * (rounds + 3))
        comms = params.commit_many(vals, [b for b in blinds])
        st = bpp.RangeStatement.init(params, comms, mins, snonce)
        w = bpp.RangeWitness.init([bpp.CommitmentOpening.new(vals[j], blinds[j]) for j in range(m)])
        use_state = state is not None and i % 4 == 1
        tr = bpp.Transcript.from_state(state.strobe.to_bytes()) if use_state else bpp.Transcript.new(LABEL)
        out.append(dict(tr=tr, st=st, w=w, ext=ext, vals=vals, blinds=blinds, mins=mins, seed=snonce, comms=comms, m=m,
                        state=state if use_state else None))
    return out


def _oracle(n, m_max, t, items):
    """the CPU oracle's bytes per item: oracle.cport for a label, oracle.pyref for a transcript state"""
    cp = cport.Params(n, m_max, t)
    want = []
    for it in items:
        if it["state"] is None:
            b, comm = cp.prove(LABEL, it["vals"], it["blinds"], it["mins"], it["seed"], it["ext"])
            assert comm == it["comms"]
        else:
            op = O.RangeParameters(n, m_max, O.PedersenGens(t))
            ost = O.RangeStatement(op, [C.decompress(c) for c in it["comms"]], it["mins"],
                                   None if it["seed"] is None else int.from_bytes(it["seed"], "little"))
            ow = O.RangeWitness([O.CommitmentOpening(it["vals"][j], [int.from_bytes(x, "little") for x in it["blinds"][j]])
                                 for j in range(it["m"])])
            b = O.prove_with_rng(it["state"].clone(), ost, ow, M.ByteStreamRng(it["ext"])).to_bytes()
        want.append(b)
    cp.close()
    return want


def _mixed(bpp, items):
    return bpp.RangeProof.prove_batch_mixed([x["tr"] for x in items], [x["st"] for x in items], [x["w"] for x in items],
                                           [x["ext"] for x in items])


def _outer_transcript():
    t0 = M.Transcript(b"outer protocol")
    t0.append_message(b"ctx", b"mixed aggregation")
    return t0


# (n, m_max, t, items per class by m); the large classes of (64, 32, 6) are kept to one proof each (the oracle's cost)
SHAPES = {
    "n64m8t1": (64, 8, 1, {1: 5, 2: 3, 4: 2, 8: 1}),
    "n8m16t3": (8, 16, 3, {1: 4, 2: 3, 4: 2, 8: 2, 16: 1}),
    "n64m32t6": (64, 32, 6, {1: 2, 2: 1, 4: 1, 8: 1, 16: 1, 32: 1}),
    # the smallest class has fewer rounds (1) than ct_back = 3 allows (n = 2, m = 1 beside m = 8: four rounds)
    "n2m8t1": (2, 8, 1, {1: 3, 2: 1, 8: 2}),
}
_CACHE = {}


def _shape(bpp, engine, key):
    if key not in _CACHE:
        n, m_max, t, per = SHAPES[key]
        params = bpp.RangeParameters.init(n, m_max, bpp.create_pedersen_gens_with_extension_degree(t), engine=engine)
        ms = [m for m, k in per.items() for _ in range(k)]
        random.Random(key).shuffle(ms)
        state = _outer_transcript() if n <= 8 else None  # (pyref only on small shapes)
        items = _items(bpp, params, n, t, ms, b"mixed-" + key.encode(), state)
        _CACHE[key] = (params, items, _oracle(n, m_max, t, items))
    return _CACHE[key]


KNOBS = [dict(ct=c, prove_parts=p, prove_fused=f, prove_subs=s) for c in (0, 1, 2) for p in (0, -1) for f in (0, 1) for s in (1, 3)]


@pytest.mark.parametrize("key", list(SHAPES))
def test_mixed_bytes_equal_oracle_under_every_knob(bpp, engine, opt, key):
    params, items, want = _shape(bpp, engine, key)
    for knobs in KNOBS:
        for name, value in knobs.items():
            opt(name, value)
        got = _mixed(bpp, items)
        for i, g in enumerate(got):
            assert not isinstance(g, Exception), (knobs, i, g)
            assert g.to_bytes() == want[i], "proof %d (m = %d) differs from the oracle under %s" % (i, items[i]["m"], knobs)


@pytest.mark.parametrize("back", [2, 3])
def test_mixed_ct_back_beyond_the_smallest_class(bpp, engine, opt, back):
    params, items, want = _shape(bpp, engine, "n2m8t1")
    opt("ct", 2)
    opt("ct_back", back)
    for fused in (0, 1):
        opt("prove_fused", fused)
        assert [g.to_bytes() for g in _mixed(bpp, items)] == want


def test_mixed_equals_one_uniform_call_per_class(bpp, engine):
    n, m_max, t = 64, 4, 3
    params = bpp.RangeParameters.init(n, m_max, bpp.create_pedersen_gens_with_extension_degree(t), engine=engine)
    ms = [1] * 40 + [2] * 20 + [4] * 20
    random.Random(7).shuffle(ms)
    items = _items(bpp, params, n, t, ms, b"per-class")
    got = [g.to_bytes() for g in _mixed(bpp, items)]
    for m in (1, 2, 4):
        idx = [i for i, x in enumerate(items) if x["m"] == m]
        one = bpp.RangeProof.prove_batch([items[i]["tr"] for i in idx], [items[i]["st"] for i in idx], [items[i]["w"] for i in idx],
                                         [items[i]["ext"] for i in idx])
        assert [got[i] for i in idx] == [p.to_bytes() for p in one]
    # a single-class batch through the new entry point equals bpp_prove_batch
    idx = [i for i, x in enumerate(items) if x["m"] == 2]
    args = ([items[i]["tr"] for i in idx], [items[i]["st"] for i in idx], [items[i]["w"] for i in idx], [items[i]["ext"] for i in idx])
    assert [g.to_bytes() for g in bpp.RangeProof.prove_batch_mixed(*args)] == [p.to_bytes() for p in bpp.RangeProof.prove_batch(*args)]


def test_mixed_ragged_schedule_across_sub_batches(bpp, engine, opt):
    """The ragged schedule over TWO sub-batches: the sorted call has 70 items, so under the default "prove_subs" a sub-batch holds
    64 and the second one is six m = 1 proofs that join two steps late -- it has no active proof at steps 0 and 1, and the prefix
    of active proofs is taken per sub-batch.  Every proof equals the oracle's bytes under every form of the round's launches."""
    n, m_max, t = 8, 4, 1
    params = bpp.RangeParameters.init(n, m_max, bpp.create_pedersen_gens_with_extension_degree(t), engine=engine)
    ms = [4] * 40 + [2] * 24 + [1] * 6
    random.Random("ragged").shuffle(ms)
    items = _items(bpp, params, n, t, ms, b"ragged")
    want = _oracle(n, m_max, t, items)
    knobs = [dict(ct=c, prove_parts=p, prove_fused=f) for c in (0, 1, 2) for p in (0, -1) for f in (0, 1)]
    for k in knobs + [dict(ct=2, ct_back=3, prove_parts=-1, prove_fused=-1)]:
        for name, value in k.items():
            opt(name, value)
        got = _mixed(bpp, items)
        for i, g in enumerate(got):
            assert not isinstance(g, Exception), (k, i, g)
            assert g.to_bytes() == want[i], "proof %d (m = %d) differs from the oracle under %s" % (i, items[i]["m"], k)


def _one_call_error(bpp, it):
    with pytest.raises(bpp.ProofError) as e:
        bpp.RangeProof.prove_batch([it["tr"]], [it["st"]], [it["w"]], [it["ext"]])
    return e.value.kind, e.value.msg


def test_mixed_per_item_errors(bpp, engine):
    n, m_max, t = 8, 4, 1
    params = bpp.RangeParameters.init(n, m_max, bpp.create_pedersen_gens_with_extension_degree(t), engine=engine)
    items = _items(bpp, params, n, t, [1, 2, 4, 1, 2, 4, 1, 2, 1, 4, 2, 1], b"errors")
    want = _oracle(n, m_max, t, items)
    bad = {}
    # an opening that does not match its commitment (found on the device)
    x = items[1]
    bad[1] = dict(x, w=bpp.RangeWitness.init([bpp.CommitmentOpening.new(x["vals"][0] ^ 1, x["blinds"][0])] +
                                             [bpp.CommitmentOpening.new(x["vals"][j], x["blinds"][j]) for j in range(1, x["m"])]))
    # a value above the bit length
    x = items[2]
    bad[2] = dict(x, w=bpp.RangeWitness.init([bpp.CommitmentOpening.new(1 << n, x["blinds"][0])] +
                                             [bpp.CommitmentOpening.new(x["vals"][j], x["blinds"][j]) for j in range(1, x["m"])]))
    # a minimum promise above the value
    x = items[4]
    bad[4] = dict(x, st=bpp.RangeStatement.init(params, x["comms"], [x["vals"][0] + 1] + [None] * (x["m"] - 1), None))
    # a seed nonce with m = 2 (the statement object is built without it: RangeStatement.init refuses it first)
    x = items[7]
    st = bpp.RangeStatement.init(params, x["comms"], x["mins"], None)
    st.seed_nonce = sb(12345)
    bad[7] = dict(x, st=st)
    # short rng bytes
    x = items[9]
    bad[9] = dict(x, ext=x["ext"][:-32])
    mixed = [bad.get(i, x) for i, x in enumerate(items)]
    got = _mixed(bpp, mixed)
    for i, g in enumerate(got):
        if i in bad:
            assert isinstance(g, bpp.ProofError), i
            assert (g.kind, g.msg) == _one_call_error(bpp, bad[i]), i
        else:
            assert g.to_bytes() == want[i], i
    # the C entry point: the return value and errbuf are the first failure's, item_status every item's code
    _params, arr, cnt, _keep = bpp.RangeProof._prove_marshal([x["tr"] for x in mixed], [x["st"] for x in mixed],
                                                            [x["w"] for x in mixed], [x["ext"] for x in mixed])
    stride = 1 + 32 * (t + 5 + 2 * 5)
    out = (ctypes.c_uint8 * (stride * cnt))()
    lens = (ctypes.c_size_t * cnt)()
    status = (ctypes.c_int * cnt)()
    err = ctypes.create_string_buffer(256)
    rc = engine.lib.bpp_prove_batch_mixed(engine.ctx, params.handle, arr, cnt, out, stride, lens, status, err, 256)
    kind, msg = _one_call_error(bpp, bad[1])
    assert rc == int(kind) and err.value.decode() == msg
    assert [status[i] for i in range(cnt)] == [int(_one_call_error(bpp, bad[i])[0]) if i in bad else 0 for i in range(cnt)]
    for i in range(cnt):
        assert lens[i] == 1 + 32 * (t + 5 + 2 * ((n * items[i]["m"]).bit_length() - 1))
        if i in bad:
            assert bytes(out[i * stride:i * stride + lens[i]]) == bytes(lens[i])


def test_mixed_round_trip_verifies_as_one_batch(bpp, engine):
    n, m_max, t = 64, 8, 2
    params = bpp.RangeParameters.init(n, m_max, bpp.create_pedersen_gens_with_extension_degree(t), engine=engine)
    ms = [1, 8, 2, 4, 1, 1, 2, 8, 4, 1, 2, 1]
    items = _items(bpp, params, n, t, ms, b"round-trip")
    proofs = _mixed(bpp, items)
    trs, sts = [bpp.Transcript.new(LABEL)] * len(items), [x["st"] for x in items]
    assert bpp.RangeProof.verify_batch(trs, sts, proofs, bpp.VerifyAction.VerifyOnly) == [None] * len(items)
    raw = bytearray(proofs[3].to_bytes())
    raw[40] ^= 1
    tampered = proofs[:3] + [bpp.RangeProof.from_bytes(bytes(raw))] + proofs[4:]
    with pytest.raises(bpp.ProofError):
        bpp.RangeProof.verify_batch(trs, sts, tampered, bpp.VerifyAction.VerifyOnly)
