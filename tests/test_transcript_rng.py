"""CPU suite: the host helpers of the transcript protocol and the transcript RNG (bpp_transcript_validate_and_append_point,
_challenge_scalar, _rng_begin, _rng_rekey, _rng_finalize, _rng_fill, _rng_scalar) against the oracle -- merlin's builder call for
call with NullRng and ByteStreamRng, protocol._challenge_scalar / _validate_and_append_point, curve.scalar_from_wide -- over the
programs tests/test_gpu_transcript_rng.py runs on the device; and the one scalar routine they share with the kernel."""
import ctypes
import importlib

import pytest

from oracle.pyref import curve as C
from oracle.pyref import merlin as M
from tests import transcript_rng_cases as TC

VERIFICATION_FAILED, INVALID_ARGUMENT = 1, 2


@pytest.fixture(scope="module")
def lib():
    return importlib.import_module("bulletproofs-plus_amd")._lib.load()


def _same(got, want, what):
    g_states, g_outs, g_void = got
    w_states, w_outs, w_void = want
    assert g_void == w_void, what
    bad = [i for i in range(len(w_states)) if g_states[i] != w_states[i]]
    assert not bad, "%s: state rows %s differ from the oracle's" % (what, bad[:8])
    for c, (g, w) in enumerate(zip(g_outs, w_outs)):
        bad = [i for i in range(len(w)) if g[i] != w[i]]
        assert not bad, "%s: output %d differs from the oracle's in rows %s" % (what, c, bad[:8])
    assert len(g_outs) == len(w_outs)


def test_every_starting_position(lib):
    makers = TC.sweep_makers()
    prog = TC.sweep_program(len(makers))
    want = TC.oracle_rows(makers, prog)
    _same(TC.helper_rows(lib, [mk().strobe.to_bytes() for mk in makers], prog), want, "169 rows")
    # the RNG operations work on a clone: the rows are the oracle's transcripts after challenge_scalar alone
    alone = TC.oracle_rows(makers, [("cscalar", b"e")])
    assert want[0] == alone[0] and want[1][-1] == alone[1][0]


def test_lengths_either_side_of_the_rate_and_the_builder(lib):
    makers = TC.edge_makers()
    start = [mk().strobe.to_bytes() for mk in makers]
    for name, prog, _ in TC.length_programs(len(makers)):
        _same(TC.helper_rows(lib, start, prog), TC.oracle_rows(makers, prog), name)
    results = {}
    for name, prog, new in TC.builder_programs(len(makers)):
        first = [M.Transcript(new).strobe.to_bytes()] * len(makers) if new is not None else start
        results[name] = TC.helper_rows(lib, first, prog)
        _same(results[name], TC.oracle_rows(makers, prog, new=new), name)
    between, plain = results["transcript ops between finalize and fill"], results["the same without them"]
    assert between[1][-1] == plain[1][-1] and between[0] != plain[0], "transcript operations must not reach the RNG"
    assert results["fill32 of 64"][1][0] != results["fill of 64"][1][0], "merlin absorbs the length before every draw"


def test_validate_and_append_point(lib):
    makers = TC.edge_makers()[:8]
    n = len(makers)
    points = TC.messages(400, n, [32] * n)
    points[2] = points[5] = bytes(32)
    prog = [("point", b"P", points), ("challenge", b"c", 32)]
    want = TC.oracle_rows(makers, prog)
    assert want[2] == [i in (2, 5) for i in range(n)]
    _same(TC.helper_rows(lib, [mk().strobe.to_bytes() for mk in makers], prog), want, "points")
    # an identity leaves the state untouched; any other point is a plain append
    st = (ctypes.c_uint8 * 203).from_buffer_copy(makers[0]().strobe.to_bytes())
    err = ctypes.create_string_buffer(128)
    assert lib.bpp_transcript_validate_and_append_point(st, b"P", 1, bytes(32), err, 128) == VERIFICATION_FAILED
    assert bytes(st) == makers[0]().strobe.to_bytes() and err.value == b"Identity element cannot be added to the transcript"
    tr = makers[0]()
    tr.append_message(b"P", points[0])
    assert lib.bpp_transcript_validate_and_append_point(st, b"P", 1, points[0], err, 128) == 0 and bytes(st) == tr.strobe.to_bytes()


def test_helpers_refuse_a_position_outside_the_block(lib):
    bad = bytearray(M.Transcript(b"x").strobe.to_bytes())
    bad[200] = 166
    st = lambda: (ctypes.c_uint8 * 203).from_buffer_copy(bytes(bad))  # noqa: E731
    out, err = (ctypes.c_uint8 * 64)(), ctypes.create_string_buffer(128)
    assert lib.bpp_transcript_validate_and_append_point(st(), b"P", 1, bytes([1]) * 32, err, 128) == INVALID_ARGUMENT
    assert lib.bpp_transcript_challenge_scalar(st(), b"e", 1, out, err, 128) == INVALID_ARGUMENT
    assert lib.bpp_transcript_rng_begin(st(), (ctypes.c_uint8 * 203)()) == INVALID_ARGUMENT
    assert lib.bpp_transcript_rng_rekey(st(), b"w", 1, bytes(32), 32) == INVALID_ARGUMENT
    assert lib.bpp_transcript_rng_finalize(st(), None) == INVALID_ARGUMENT
    assert lib.bpp_transcript_rng_fill(st(), out, 32) == INVALID_ARGUMENT
    assert lib.bpp_transcript_rng_scalar(st(), out, err, 128) == INVALID_ARGUMENT


def test_the_shared_scalar_routine_at_zero_and_around_l():
    """top_scalar_from_wide (transcript_ops.h) is the one routine behind challenge_scalar and Scalar::random in the kernel, in its host
    model and in the host helpers.  THIS IS THE ONLY PLACE THE ZERO-SCALAR RULE CAN BE REACHED: no input is known whose 64 squeezed
    bytes reduce to zero, so the device tests cannot void a row that way; the kernel's path behind the flag is the void tail that the
    up-front void rows already take.  64 zero bytes and the 64-byte encoding of l give zero with the flag set; l - 1 and l + 1 do not."""
    pkg = importlib.import_module("bulletproofs-plus_amd")
    ht = ctypes.CDLL(pkg._build.build_hosttest())
    ht.ht_top_scalar_from_wide.restype = ctypes.c_uint32
    cases = [(0, 0, 1), (C.L, 0, 1), (C.L - 1, C.L - 1, 0), (C.L + 1, 1, 0), (2 * C.L, 0, 1), (2 ** 512 - 1, (2 ** 512 - 1) % C.L, 0),
             ((2 ** 512 - 1) // C.L * C.L, 0, 1), (1 << 256, (1 << 256) % C.L, 0)]
    for value, want, want_zero in cases:
        out = (ctypes.c_uint8 * 32)()
        zero = ht.ht_top_scalar_from_wide(value.to_bytes(64, "little"), out)
        assert (int.from_bytes(bytes(out), "little"), zero) == (want, want_zero), hex(value)
        assert C.scalar_from_wide(value.to_bytes(64, "little")) == want
