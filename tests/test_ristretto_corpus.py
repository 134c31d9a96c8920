"""CPU suite: the decoding corpus (tests/ristretto_corpus.py) is what it claims to be, the oracle and the host compile of both
decoders of csrc/point.h agree with it member by member, and the oracle proves and verifies under caller-supplied Pedersen
bases (the reference of tests/test_gpu_custom_bases.py)."""
import collections
import ctypes
import importlib

import pytest

from oracle.pyref import curve as C
from oracle.pyref import merlin as M
from oracle.pyref import protocol as O
from tests import helpers as H
from tests import ristretto_corpus as R


@pytest.fixture(scope="module")
def ht():
    pkg = importlib.import_module("bulletproofs-plus_amd")
    return ctypes.CDLL(pkg._build.build_hosttest())


def test_constructive_members_land_in_their_class():
    for name, b, want in R.CONSTRUCTIVE:
        assert len(b) == 32 and R.classify(b) == want, (name, R.classify(b), want)
    assert {c for _, _, c in R.CONSTRUCTIVE} == set(R.CLASSES)
    assert len({b for _, b, _ in R.CONSTRUCTIVE}) == len(R.CONSTRUCTIVE)  # (some are among the RFC's strings too)
    # the members that exactly one condition refuses: the residue of a non-canonical one, the negation of a negative one are points
    for name in ("p+0", "p+4", "p+6"):
        b = dict(R.NAMED)[name]
        assert R.classify(R.enc(int.from_bytes(b, "little") - R.P)) == "valid", name
    for name in ("p-4", "p-6"):
        b = dict(R.NAMED)[name]
        assert R.classify(R.enc(R.P - int.from_bytes(b, "little"))) == "valid", name
    assert all(R.classify(b) != "valid" for _, b in R.FIXED)


def test_classifier_equals_the_oracle_on_the_whole_corpus():
    for name, b in R.CORPUS:
        pt = C.decompress(b)
        assert (R.classify(b) == "valid") == (pt is not None), name
        if pt is not None:
            assert pt.compress() == b, name


def test_random_part_holds_every_class_it_can():
    n = collections.Counter(R.classify(b) for _, b in R.RANDOM)
    assert set(n) == {"valid", "nonsquare", "t_negative"}, n
    assert all(v >= 60 for v in n.values()), n


def test_host_build_of_both_decoders_on_the_corpus(ht):
    for name, b in R.CORPUS:
        valid = R.classify(b) == "valid"
        o1, o2 = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
        assert (ht.ht_decompress_compress(b, o1) == 1) == valid, ("ristretto_decompress", name, R.classify(b))
        assert (ht.ht_decompress_lean(b, o2) == 1) == valid, ("ristretto_decompress_lean", name, R.classify(b))
        if valid:
            assert o1.raw == b and o2.raw == b, name


@pytest.mark.parametrize("which", ["random", "edge"])
def test_oracle_round_trip_under_custom_bases(which):
    """prove -> verify under the caller's bases; the same proofs are refused under the default bases and default-base proofs
    under the caller's (VerificationFailed: the transcript binds H and G, the final check every commitment)"""
    pc = H.custom_pedersen_gens(2, which)
    assert pc.h_base_compressed != O.PedersenGens(2).h_base_compressed
    c = H.make_oracle_batch(8, [1, 2], 2, seed=b"custom-cpu-" + which.encode(), pc_gens=pc)
    masks, tr = H.oracle_verify_trace(c, action=1)
    assert tr["msm_result"] == bytes(32)
    assert masks[0] == [H.sb(x) for x in c.expected_masks[0]] and masks[1] is None
    assert len(set(c.expected_masks[0])) == 2  # fresh blinding per generator: a swapped G_k would show
    d = H.make_oracle_batch(8, [1, 2], 2, seed=b"custom-cpu-" + which.encode())
    for proofs, sts in ((c.o_proofs, H.restate(c, d.o_params)), (d.o_proofs, H.restate(d, c.o_params))):
        with pytest.raises(O.ProofError) as e:
            O.verify([M.Transcript(c.label) for _ in proofs], sts, proofs, O.VERIFY_ONLY)
        assert e.value.kind == O.VERIFICATION_FAILED
