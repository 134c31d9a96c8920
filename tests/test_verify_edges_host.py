"""CPU suite: the forced-challenge families of tests/helpers.py are what they claim, on the oracle alone.

An honest oracle prover under a forced row of challenges gives a proof that the oracle's verifier accepts under the same row, for
every row of every family (the protocol is complete for any non-zero challenges with y != 1); tests/test_gpu_verify_edges.py then
holds the device's PASS 2 to that.  Nothing here is dropped to make it pass: a rejected case is a bug in the builder."""
import pytest

from oracle.pyref import curve as C
from oracle.pyref import protocol as O
from tests import helpers as H

L = C.L
SHAPES = [(8, 1, 1), (8, 2, 2)]


def test_edge_scalars_are_the_listed_values():
    names = [n for n, _ in H.EDGE_SCALARS]
    vals = dict(H.EDGE_SCALARS)
    assert len(names) == len(set(names)) == 17 and len(set(vals.values())) == 17
    assert all(0 < v < L for v in vals.values())
    assert [vals[k] for k in ("1", "2", "l-1", "l-2", "2^252", "(l+1)/2", "(l-1)/2", "2^29-1", "2^29", "2^58", "2^232-1")] == \
        [1, 2, L - 1, L - 2, 2**252, (L + 1) // 2, (L - 1) // 2, 2**29 - 1, 2**29, 2**58, 2**232 - 1]
    assert 2 * vals["(l+1)/2"] % L == 1 and (2 * vals["(l-1)/2"] + 1) % L == 0
    # the ten of the first experiment come first
    assert set(names[:10]) == {"1", "2", "l-1", "l-2", "2^252", "(l+1)/2", "mont^-1(1)", "mont^-1(l-1)", "mont^-1(2^252-1)",
                               "mont^-1(2^252)"}


def test_montgomery_preimages_map_to_their_images():
    """x * 2^261 mod l is what the name says: 1, l-1, l-2 (one, minus one, and the value next to it, in Montgomery form), 2^252-1
    (eight limbs of 29 one-bits and a full top limb), 2^252 (the top limb's last bit alone), 2^29-1 (one full limb)"""
    vals = dict(H.EDGE_SCALARS)
    assert sorted(H.EDGE_MONT_IMAGES) == sorted(n for n in vals if n.startswith("mont^-1"))
    for name, image in H.EDGE_MONT_IMAGES.items():
        assert vals[name] * (1 << 261) % L == image, name
    limbs = lambda v: [(v >> (29 * i)) & (2**29 - 1) for i in range(9)]
    assert limbs((1 << 252) - 1) == [2**29 - 1] * 8 + [2**20 - 1]
    assert limbs(vals["mont^-1(2^29-1)"] * (1 << 261) % L) == [2**29 - 1] + [0] * 8


def test_forced_challenges_restores_and_records():
    orig = O._challenge_scalar
    with pytest.raises(RuntimeError):
        with H.forced_challenges([[5, None, 7, 7, 7, None]]) as rec:
            assert O._challenge_scalar is not orig
            raise RuntimeError
    assert O._challenge_scalar is orig
    c = H.edge_challenge_case(8, 1, 1, [5, None, 7, None, 7, None], b"restore")
    assert O._challenge_scalar is orig
    assert c.oracle_error is None and c.expected_masks == c.witness_masks
    assert [c.values[k] for k in (0, 2, 4)] == [5, 7, 7]
    # the transcript is still advanced: the positions left alone are hashes of a transcript that holds the proof.  z follows A
    # alone, which no challenge enters, so it is the unforced run's; the later ones follow points made with the forced values
    free = H.edge_challenge_case(8, 1, 1, [None] * 6, b"restore")
    assert all(v > 2**200 for v in (c.values[1], c.values[3], c.values[5]))
    assert free.values[1] == c.values[1] and free.values[3] != c.values[3] and free.values[5] != c.values[5]
    assert free.oracle_error is None and free.expected_masks == free.witness_masks
    # a second proof in the block keeps its hashed values when `rows` holds one row
    with H.forced_challenges([[3] * 6]) as rec:
        masks = O.verify([H.M.Transcript(H.LABEL), H.M.Transcript(H.LABEL)], [free.o_statement_private] * 2, [free.o_proof] * 2, 2)
    assert rec.returned[0] == [3] * 6 and rec.returned[1] == free.values
    assert [H.sb(x) for x in masks[1]] == free.witness_masks[0] != [H.sb(x) for x in masks[0]]


@pytest.mark.parametrize("n,m,t", SHAPES)
def test_families_are_complete(n, m, t):
    """every (position class, edge value) is there, y = 1 alone left out, plus the two all-edge rows"""
    fams = H.edge_challenge_families(n, m, t)
    rounds = (n * m).bit_length() - 1
    assert sorted(fams) == sorted(H.EDGE_POSITION_CLASSES + ("all_edge",))
    where = {"y": [0], "z": [1], "e_all": list(range(2, 2 + rounds)), "e_first": [2], "e_last": [1 + rounds], "e_final": [2 + rounds]}
    for cls in H.EDGE_POSITION_CLASSES:
        want = [(name, v) for name, v in H.EDGE_SCALARS if not (cls == "y" and v == 1)]
        assert len(want) == (16 if cls == "y" else 17)
        assert [c.name for c in fams[cls]] == ["%s=%s" % (cls, name) for name, _ in want]
        for c, (_, v) in zip(fams[cls], want):
            assert c.row == [v if k in where[cls] else None for k in range(rounds + 3)], c.name
    a, b = fams["all_edge"]
    assert a.row == [L - 1] * (rounds + 3) and b.row == [(L - 1, 1)[k & 1] for k in range(rounds + 3)]
    assert sum(len(v) for v in fams.values()) == 6 * 17 - 1 + 2


@pytest.mark.parametrize("family", H.EDGE_POSITION_CLASSES + ("all_edge",))
@pytest.mark.parametrize("n,m,t", SHAPES)
def test_oracle_accepts_every_case(n, m, t, family):
    """RecoverAndVerify (action 1: the final check runs) for m == 1, where it also returns the witness's blinding factors;
    VerifyOnly for aggregated statements, which carry no nonce"""
    for c in H.edge_challenge_families(n, m, t)[family]:
        assert c.oracle_error is None, "%s: %s" % (c.name, c.oracle_error)
        assert c.action == (1 if m == 1 else 0)
        assert c.values == [v if v is not None else c.values[k] for k, v in enumerate(c.row)], c.name
        assert len(c.rng_outputs) == 1 and len(c.rng_outputs[0]) == 32
        if m == 1:
            assert c.expected_masks == c.witness_masks and len(c.expected_masks[0]) == t, c.name
        else:
            assert c.expected_masks == [None] == c.witness_masks, c.name
        # the forced values are what the verifier computed with: unforced, the same proof is rejected
    c = H.edge_challenge_families(n, m, t)[family][-1]
    _, err, _ = H.oracle_verify_forced(c, [None] * len(c.row), 0)
    assert err is not None and err.kind == O.VERIFICATION_FAILED


@pytest.mark.parametrize("n,m,t", SHAPES)
def test_y_one_is_rejected_by_the_oracle(n, m, t):
    """at y = 1 the verifier's y_sum = y (y^mn - 1) (y - 1)^-1 is 0 under inverse(0) = 0, not mn"""
    c = H.edge_y_one_case(n, m, t)
    assert c.values[0] == 1
    assert c.oracle_error is not None and c.oracle_error.kind == O.VERIFICATION_FAILED
