"""CPU test of the agreement rule of "verify_check" (bpp_verify_check_resolve, include/bpp.h): pure host code, no device.
passes[0 .. n) are one group's outcomes in pass order; two outcomes agree when code, tier and index are the same."""
import ctypes
import importlib
import itertools

NOT_RECHECKED, CONFIRMED, UPHELD, OVERTURNED, UNDECIDED, PENDING = 0, 1, 2, 3, 4, 5
SELF_CHECK, TIER_ENGINE = -5, 255
OK = (0, 0, 0, b"")
MSM = (1, 7, 0, b"Range proof batch not valid")
PASS1 = (1, 5, 2, b"Identity element cannot be added to the transcript / transcript challenge cannot be zero")
PASS2 = (2, 6, 1, b"A proof member was not the canonical encoding of a point")
PASS2_OTHER_INDEX = (2, 6, 3, b"A proof member was not the canonical encoding of a point")
DEGREE = (2, 2, 0, b"Inconsistent extension degree")


def _resolve(outcomes):
    pkg = importlib.import_module("bulletproofs-plus_amd")
    pkg._build.build()
    lib = pkg._lib.load()
    R = pkg._lib.ShardResult
    arr = (R * len(outcomes))()
    for r, (code, tier, index, msg) in zip(arr, outcomes):
        r.code, r.tier, r.rank, r.index, r.msg = code, tier, -1, index, msg
    out, kind = R(), ctypes.c_int(-99)
    out.code = 77  # (must stay as it is while the answer is PENDING)
    rc = lib.bpp_verify_check_resolve(arr, len(outcomes), ctypes.byref(out), ctypes.byref(kind))
    return rc, kind.value, (out.code, out.tier, out.index, out.msg)


def test_outcomes_without_a_device_tier_finding_stand():
    for first in (OK, DEGREE, (-1, TIER_ENGINE, 0, b"engine fault")):
        for rest in ([], [MSM], [MSM, PASS1]):
            assert _resolve([first] + rest) == (0, NOT_RECHECKED, first)


def test_one_pass_with_a_device_finding_asks_for_the_next():
    for first in (MSM, PASS1, PASS2):
        rc, kind, out = _resolve([first])
        assert (rc, kind) == (1, PENDING) and out[0] == 77


def test_pass_two_confirms_or_asks_for_the_third():
    for first in (MSM, PASS1, PASS2):
        assert _resolve([first, first]) == (0, CONFIRMED, first)
        assert _resolve([first, first, OK]) == (0, CONFIRMED, first)  # (a third outcome is not looked at)
        for second in (OK, MSM, PASS1, PASS2, PASS2_OTHER_INDEX):
            if second[:3] != first[:3]:
                rc, kind, out = _resolve([first, second])
                assert (rc, kind) == (1, PENDING) and out[0] == 77


def test_every_pattern_of_three_passes():
    kinds = (OK, MSM, PASS1, PASS2, PASS2_OTHER_INDEX)
    for a, b, c in itertools.product(kinds, repeat=3):
        rc, kind, out = _resolve([a, b, c])
        assert rc == 0
        if a is OK:
            assert (kind, out) == (NOT_RECHECKED, a)
        elif a[:3] == b[:3]:
            assert (kind, out) == (CONFIRMED, a)
        elif a[:3] == c[:3]:
            assert (kind, out) == (UPHELD, a)
        elif b[:3] == c[:3]:
            assert (kind, out) == (OVERTURNED, c)  # may be Ok: a false rejection overturned
        else:
            assert kind == UNDECIDED and out[0] == SELF_CHECK and out[1] == TIER_ENGINE
            for o in (a, b, c):  # the message names the three outcomes
                assert b"%d/%d/%d" % o[:3] in out[3], out[3]


def test_agreement_ignores_the_message_but_not_the_index():
    same_but_text = (MSM[0], MSM[1], MSM[2], b"other words")
    assert _resolve([MSM, same_but_text]) == (0, CONFIRMED, MSM)
    assert _resolve([PASS2, PASS2_OTHER_INDEX])[1] == PENDING
    assert _resolve([PASS2, PASS2_OTHER_INDEX, PASS2_OTHER_INDEX]) == (0, OVERTURNED, PASS2_OTHER_INDEX)


def test_bad_arguments():
    pkg = importlib.import_module("bulletproofs-plus_amd")
    lib = pkg._lib.load()
    R = pkg._lib.ShardResult
    arr, out, kind = (R * 3)(), R(), ctypes.c_int()
    assert lib.bpp_verify_check_resolve(None, 1, ctypes.byref(out), ctypes.byref(kind)) == 2
    assert lib.bpp_verify_check_resolve(arr, 0, ctypes.byref(out), ctypes.byref(kind)) == 2
    assert lib.bpp_verify_check_resolve(arr, 4, ctypes.byref(out), ctypes.byref(kind)) == 2
    assert lib.bpp_verify_check_resolve(arr, 1, None, ctypes.byref(kind)) == 2
    assert lib.bpp_verify_check_resolve(arr, 1, ctypes.byref(out), None) == 2
