"""CPU suite: merlin's own operations on a 203-byte state (bpp_transcript_append_message / bpp_transcript_challenge_bytes, host
only) against oracle.pyref.merlin.Transcript, with messages either side of the STROBE rate; the Python mirror's Transcript
operations; a state whose position lies outside the block is refused, as the upload refuses it."""
import ctypes
import importlib

import pytest

from oracle.pyref import merlin as M
from tests import transcript_sweep as TS

LABEL, CTX_LABEL, CTX = b"outer protocol v1", b"block-context", bytes(range(7, 64))
MSG_LENS = [0, 1, 165, 166, 167, 400]  # STROBE-128's rate is 166 bytes
CHALLENGE_LENS = [1, 32, 64, 200]


def _lib():
    return importlib.import_module("bulletproofs-plus_amd")._lib.load()


def _buf(b):
    return (ctypes.c_uint8 * max(len(b), 1)).from_buffer_copy(b if len(b) else b"\0")


def _oracle(context):
    t = M.Transcript(LABEL)
    if context:
        t.append_message(CTX_LABEL, CTX)
    return t


def _msg(n):
    return bytes((37 * i + n) & 0xff for i in range(n))


@pytest.mark.parametrize("context", [False, True], ids=["label-made", "with-context"])
def test_append_and_challenge_equal_the_oracle(context):
    lib = _lib()
    for n in MSG_LENS:
        for c in CHALLENGE_LENS:
            o = _oracle(context)
            st = _buf(o.strobe.to_bytes())
            o.append_message(b"msg", _msg(n))
            assert lib.bpp_transcript_append_message(st, _buf(b"msg"), 3, _buf(_msg(n)), n) == 0
            assert bytes(st) == o.strobe.to_bytes(), (n, c)
            out = (ctypes.c_uint8 * c)()
            assert lib.bpp_transcript_challenge_bytes(st, _buf(b"chal"), 4, out, c) == 0
            assert bytes(out) == o.challenge_bytes(b"chal", c), (n, c)
            assert bytes(st) == o.strobe.to_bytes(), (n, c)
            # and the state goes on: a second message, a second challenge
            o.append_message(b"", _msg(n)[::-1])
            assert lib.bpp_transcript_append_message(st, None, 0, _buf(_msg(n)[::-1]), n) == 0
            assert lib.bpp_transcript_challenge_bytes(st, _buf(b"after"), 5, out, c) == 0
            assert bytes(out) == o.challenge_bytes(b"after", c) and bytes(st) == o.strobe.to_bytes(), (n, c)


def test_label_made_state_is_transcript_new():
    lib = _lib()
    st = (ctypes.c_uint8 * 203)()
    assert lib.bpp_transcript_new(_buf(LABEL), len(LABEL), st) == 0
    o = M.Transcript(LABEL)
    assert bytes(st) == o.strobe.to_bytes()
    o.append_message(CTX_LABEL, CTX)
    assert lib.bpp_transcript_append_message(st, _buf(CTX_LABEL), len(CTX_LABEL), _buf(CTX), len(CTX)) == 0
    assert bytes(st) == o.strobe.to_bytes()


def test_transcript_new_at_every_starting_position():
    """bpp_transcript_new over the sweep's 166 labels (lengths 0 .. 165: every position of the block) and labels longer than a block;
    one message and one challenge from each of those states"""
    lib = _lib()
    assert sorted(M.Transcript(TS.label_of(n)).strobe.pos for n in range(166)) == list(range(166))
    for n in list(range(166)) + [166, 167, 400]:
        label = TS.label_of(n)
        st = (ctypes.c_uint8 * 203)()
        assert lib.bpp_transcript_new(_buf(label), n, st) == 0
        o = M.Transcript(label)
        assert bytes(st) == o.strobe.to_bytes(), n
        o.append_message(b"msg", _msg(40))
        assert lib.bpp_transcript_append_message(st, _buf(b"msg"), 3, _buf(_msg(40)), 40) == 0
        assert bytes(st) == o.strobe.to_bytes(), n
        out = (ctypes.c_uint8 * 32)()
        assert lib.bpp_transcript_challenge_bytes(st, _buf(b"chal"), 4, out, 32) == 0
        assert bytes(out) == o.challenge_bytes(b"chal", 32) and bytes(st) == o.strobe.to_bytes(), n


@pytest.mark.parametrize("pos", [166, 167, 255])
def test_a_state_outside_the_block_is_refused(pos):
    lib = _lib()
    good = _oracle(True).strobe.to_bytes()
    bad = bytearray(good)
    bad[200] = pos
    st = _buf(bytes(bad))
    out = (ctypes.c_uint8 * 32)()
    assert lib.bpp_transcript_append_message(st, _buf(b"m"), 1, _buf(b"x"), 1) == 2  # BPP_ERR_INVALID_ARGUMENT
    assert lib.bpp_transcript_challenge_bytes(st, _buf(b"c"), 1, out, 32) == 2
    assert bytes(st) == bytes(bad) and bytes(out) == bytes(32)  # nothing was touched
    ok = bytearray(good)
    ok[200] = 165  # the last position inside the block
    assert lib.bpp_transcript_append_message(_buf(bytes(ok)), _buf(b"m"), 1, _buf(b"x"), 1) == 0
    assert lib.bpp_transcript_append_message(None, _buf(b"m"), 1, _buf(b"x"), 1) == 2
    assert lib.bpp_transcript_challenge_bytes(_buf(good), _buf(b"c"), 1, None, 32) == 2


def test_python_transcript_operations():
    bpp = importlib.import_module("bulletproofs-plus_amd")
    o = M.Transcript(LABEL)
    t = bpp.Transcript.new(LABEL)
    assert t.state is None
    t.append_message(CTX_LABEL, CTX)  # a label-only transcript materialises its state first
    o.append_message(CTX_LABEL, CTX)
    assert t.state == o.strobe.to_bytes() and t.label is None
    t.append_u64(b"height", 2**40 + 5)
    o.append_u64(b"height", 2**40 + 5)
    assert t.strobe_state() == o.strobe.to_bytes()
    for n in CHALLENGE_LENS:
        assert t.challenge_bytes(b"c", n) == o.challenge_bytes(b"c", n)
    assert t.state == o.strobe.to_bytes()
    c = t.clone()
    c.append_message(b"x", b"y")
    assert t.state == o.strobe.to_bytes()  # a clone is its own transcript
    s = bpp.Transcript.from_state(o.strobe.to_bytes())
    assert s.challenge_bytes(b"again", 16) == o.challenge_bytes(b"again", 16)
    bad = bytearray(o.strobe.to_bytes())
    bad[200] = 166
    with pytest.raises(bpp.ProofError):
        bpp.Transcript.from_state(bytes(bad)).append_message(b"m", b"x")


def test_advance_needs_one_object_per_item():
    """checked before anything reaches the engine: no device needed"""
    bpp = importlib.import_module("bulletproofs-plus_amd")
    t = bpp.Transcript.new(LABEL)
    with pytest.raises(bpp.ProofError) as e:
        bpp.api._check_advance([t, bpp.Transcript.new(LABEL), t])
    assert e.value.kind == bpp.ProofErrorKind.InvalidArgument
    bpp.api._check_advance([bpp.Transcript.new(LABEL), bpp.Transcript.new(LABEL)])
