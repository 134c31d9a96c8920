"""CPU suite: the sweep fixture of tests/transcript_sweep.py really puts the range proof's sponge at every position of the block.

tests/test_gpu_transcript_alignment.py compares the device's sponges with the oracle over that fixture; what it is worth depends on
the fixture reaching every (absorb length, start position) pair, every crossing of the block boundary and both branches of the
`pos != 0` test of the first operation that carries the C flag.  The figures are asserted here, on the oracle's own sponge with
its _absorb and _run_f wrapped for the length of a test, so that a shortened sweep fails here and not silently there."""
import pytest

from oracle.pyref import merlin as M
from oracle.pyref import protocol as O
from tests import transcript_sweep as TS
from tests.helpers import replay_verifier_state

# what the range proof absorbs before its first challenge, by length: labels of 1 (H, G, N, T, M, A, y), 2 (Ci and every operation's
# header), 3 ("rng"), 7 ("dom-sep"), 18 ("vi - minimum_value"); the u32 length (4), a u64 (8), the domain separator's 25 bytes, a point (32)
ABSORB_LENGTHS = {1, 2, 3, 4, 7, 8, 18, 25, 32}


def test_the_labels_are_the_166_starting_positions():
    labels = [TS.label_of(length) for length in range(TS.RATE)]
    assert [len(x) for x in labels] == list(range(166)) and TS.RATE == 166
    assert all(len(set(x)) > 1 for x in labels[2:])  # not constant
    assert TS.start_positions() == [(28 + length) % 166 for length in range(166)]
    assert len(set(TS.start_positions())) == 166
    assert sorted(TS.ORDER) == list(range(166))
    assert all(abs(a - b) > 8 for a, b in zip(TS.ORDER, TS.ORDER[1:]))  # neighbours in the call are not neighbours in the block


@pytest.mark.parametrize("shape", ["A", "B"])
def test_the_sweep_is_what_it_says(shape):
    c = TS.sweep(shape)
    s = TS.SHAPES[shape]
    assert len(c.items) == 166 and sorted(c.lengths) == list(range(166)) and sorted(c.positions) == list(range(166))
    assert c.labels == [TS.label_of(length) for length in c.lengths] and [st[200] for st in c.states] == c.positions
    top = 1 << (s["n"] - 1)
    flat = [v for values in c.values for v in values]
    assert all(0 <= v < 2 * top for v in flat) and any(v & top for v in flat) and (2 * top - 1) in flat and 0 in flat
    assert all(len(set(rs)) == s["t"] for bl in c.blindings for rs in bl)  # a blinding of its own per generator
    assert all((x is not None) == s["seed_nonce"] for x in c.seeds)
    assert all((x is not None) == s["promise"] for mins in c.mins for x in mins)
    assert all(len(it["commitments"]) == s["m"] and it["proof"][0] == s["t"] for it in c.items)
    assert len({it["proof"] for it in c.items}) == 166
    assert TS.sweep(shape) is c  # built once


@pytest.mark.parametrize("shape", ["A", "B"])
def test_the_sweep_reaches_every_alignment(shape, monkeypatch):
    """RangeProofTranscript::new + challenges_y_z over the 166 labels: 9 absorb lengths x 166 positions = 1494 pairs, of which
    1 + 2 + 3 + 4 + 7 + 8 + 18 + 25 + 32 = 100 reach or cross the end of the block; the first operation with the C flag finds the
    sponge at 165 positions other than 0 (it permutes once more) and, for one label, at 0 (it does not)."""
    c = TS.sweep(shape)
    pc = O.PedersenGens(c.t)
    pairs, first_c, first_c_main = set(), [], []
    log = TS.log_sponge(monkeypatch)
    for k in range(len(c.items)):
        tr = M.Transcript(c.labels[k])
        assert tr.strobe.pos == c.positions[k]
        del log.absorbs[:], log.c_ops[:], log.run_f[:]  # (Transcript::new is the caller's: the range proof starts here)
        st = type("S", (), {"commitments_compressed": c.commitments[k], "minimum_value_promises": c.mins[k]})
        rpt = O.RangeProofTranscript(tr, pc.h_base_compressed, pc.g_base_compressed_vec, c.n, c.t, c.m, st, None, M.NullRng())
        rpt.challenges_y_z(O.RangeProof.from_bytes(c.raw[k]).a)
        y = next(i for i, (s, _, _) in enumerate(log.c_ops) if s is tr.strobe)  # the first challenge: up to here the position is the caller's
        upto = log.absorbs[:log.c_ops[y][2]]  # (what follows it starts at a fixed position)
        pairs.update(upto)
        first_c.append(log.c_ops[0][1])  # the TranscriptRng cloned inside RangeProofTranscript::new: its KEY operation
        first_c_main.append(log.c_ops[y][1])  # the challenge y on the transcript itself
    assert {n for n, _ in pairs} == ABSORB_LENGTHS
    assert len(pairs) == 1494 == 9 * 166
    assert len([1 for n, pos in pairs if pos + n >= 166]) == 100 == sum(ABSORB_LENGTHS)
    for seen in (first_c, first_c_main):
        assert len({p for p in seen if p != 0}) == 165 and sorted(seen) == list(range(166))
        assert seen.count(0) == 1  # the one start from which no permutation is forced


def test_the_replay_leaves_the_oracles_verifier_state():
    """replay_verifier_state (the hash-only PASS 1 that the GPU tests take their expected states from) against the oracle's own
    verify() on a few positions of shape A, the block's two ends among them"""
    c = TS.sweep("A")
    o_params = O.RangeParameters(c.n, c.m, O.PedersenGens(c.t))
    for k in [c.positions.index(p) for p in (0, 1, 164, 165)] + [0]:
        st, _ = TS.oracle_statement(c, k, o_params)
        tr = M.Transcript(c.labels[k])
        masks = O.verify([tr], [st], [O.RangeProof.from_bytes(c.raw[k])], 1)
        assert [int.to_bytes(x, 32, "little") for x in masks[0]] == c.blindings[k][0]
        got = replay_verifier_state(M.Transcript(c.labels[k]), c.n, c.t, o_params.pc_gens, c.commitments[k], c.mins[k], c.raw[k])
        assert got == tr.strobe.to_bytes(), c.describe(k)
