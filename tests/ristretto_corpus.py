"""One corpus of 32-byte strings for every ristretto255 decoder of the product: the host compile of csrc/point.h
(tests/test_ristretto_corpus.py) and the three device forms (tests/test_gpu_decode.py).

RFC 9496 4.3.1 refuses an encoding for one of five reasons: it is not canonical, s is negative, v u2^2 is not a square, t is
negative, y is zero.  Random strings almost never meet the first, second or fifth alone, and never the edges of any, so the
members here are CONSTRUCTED: for every condition there are strings that this condition alone refuses (p + 4 is only not
canonical: its residue 4 is a point; p - 1 is canonical, even, square and has t = 0: only y = 0 refuses it).  A decoder that
dropped one check accepts them.

classify() restates the RFC's conditions in plain big-int arithmetic with square roots of its own (Euler's criterion and the
p = 5 mod 8 root), not through oracle.pyref.curve.decompress; tests/test_ristretto_corpus.py pins the two against each other."""
import hashlib

from oracle.pyref import curve as C

P = 2**255 - 19
_D = -121665 * pow(121666, P - 2, P) % P
_I = pow(2, (P - 1) // 4, P)  # a square root of -1

CLASSES = ("bit255", "ge_p", "negative", "w_zero", "nonsquare", "y_zero", "t_negative", "valid")


def enc(s):
    """the 32 little-endian bytes of s < 2^256 (no reduction: s >= p stays non-canonical)"""
    return int(s).to_bytes(32, "little")


def _sqrt(a):
    """a root of the non-zero square a (p = 5 mod 8): a^((p+3)/8), times sqrt(-1) if that is a root of -a"""
    x = pow(a, (P + 3) // 8, P)
    if x * x % P != a:
        x = x * _I % P
    assert x * x % P == a
    return x


def classify(b32):
    """which condition of RFC 9496 4.3.1 refuses b32, tested in the RFC's order; "valid" if none does"""
    assert len(b32) == 32
    s = int.from_bytes(b32, "little")
    if s >> 255:
        return "bit255"
    if s >= P:
        return "ge_p"
    if s & 1:
        return "negative"
    ss = s * s % P
    u1, u2 = (1 - ss) % P, (1 + ss) % P
    v = (-_D * u1 * u1 - u2 * u2) % P
    w = v * u2 * u2 % P
    if w == 0:  # SQRT_RATIO_M1(1, 0) reports "not a square"; kept apart because the decoders' root formulas differ exactly here
        return "w_zero"
    if pow(w, (P - 1) // 2, P) != 1:
        return "nonsquare"
    invsqrt = _sqrt(pow(w, P - 2, P))
    if invsqrt & 1:
        invsqrt = P - invsqrt  # SQRT_RATIO_M1 returns the non-negative root
    den_x = invsqrt * u2 % P
    den_y = invsqrt * den_x % P * v % P
    x = 2 * s * den_x % P
    if x & 1:
        x = P - x
    y = u1 * den_y % P
    if y == 0:
        return "y_zero"
    if (x * y % P) & 1:
        return "t_negative"
    return "valid"


_UNIFORM = [C.from_uniform_bytes(hashlib.shake_256(b"dec-uniform-%d" % i).digest(64)).compress() for i in range(3)]
_BASE = C.BASEPOINT.compress()

# (name, bytes, the class it must land in)
CONSTRUCTIVE = [
    ("identity", enc(0), "valid"), ("4", enc(4), "valid"), ("6", enc(6), "valid"), ("20", enc(20), "valid"),
    ("p-3", enc(P - 3), "valid"), ("basepoint", _BASE, "valid"),
    ("uniform0", _UNIFORM[0], "valid"), ("uniform1", _UNIFORM[1], "valid"), ("uniform2", _UNIFORM[2], "valid"),
    ("p+0", enc(P), "ge_p"), ("p+4", enc(P + 4), "ge_p"), ("p+6", enc(P + 6), "ge_p"), ("p+18", enc(P + 18), "ge_p"),
    ("p+1", enc(P + 1), "ge_p"),
    # p + 4 and p + 6 are odd numbers: a decoder that tests the sign on the BYTES (csrc/point.h does) refuses them twice.  p + 3 is
    # even and its residue 3 decodes like p - 3 once the sign is not looked at: there the canonical check alone refuses it
    ("p+3", enc(P + 3), "ge_p"),
    ("basepoint|bit255", _BASE[:31] + bytes([_BASE[31] | 0x80]), "bit255"), ("2^255", enc(1 << 255), "bit255"),
    ("1", enc(1), "negative"), ("p-4", enc(P - 4), "negative"), ("p-6", enc(P - 6), "negative"),
    ("p-sqrt(-1)", enc(P - C.SQRT_M1), "negative"),
    ("sqrt(-1)", enc(C.SQRT_M1), "w_zero"),
    ("p-1", enc(P - 1), "y_zero"),
    ("8", enc(8), "nonsquare"), ("12", enc(12), "nonsquare"), ("14", enc(14), "nonsquare"),
    ("2", enc(2), "t_negative"), ("10", enc(10), "t_negative"), ("16", enc(16), "t_negative"), ("p-7", enc(P - 7), "t_negative"),
]

# RFC 9496 appendix A.2 (the strings of tests/test_oracle_kats.py) and the all-ones string: refused, whatever the class
RFC_A2 = ["00ffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff",
          "ffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff7f",
          "f3ffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff7f",
          "edffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff7f",
          "0100000000000000000000000000000000000000000000000000000000000000",
          "01ffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff7f",
          "ed57ffd8c914fb201471d1c3d245ce3c746fcbe63a3679d51b6a516ebebe0e20",
          "c34c4e1826e5d403b78e246e88aa051c36ccf0aafebffe137d148a2bf9104562",
          "26948d35ca62e643e26a83177332e6b6afeb9d08e4268b650f1f5bbd8d81d371",
          "4eac077a713c57b4f4397629a4145982c661f48044dd3f96427d40b147d9742f",
          "ecffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff7f",
          "47cfc5497c53dc8e61c91d17fd626ffb1c49e2bca94eed052281b510b1117a24"]
FIXED = [("rfc-a2-%d" % i, bytes.fromhex(h)) for i, h in enumerate(RFC_A2)] + [("ff..ff", b"\xff" * 32)]


def _random_member(i):
    b = bytearray(hashlib.shake_256(b"dec-%d" % i).digest(32))
    b[0] &= 0xfe   # non-negative
    b[31] &= 0x7f  # below 2^255 (and, but for 19 values, below p)
    return bytes(b)


RANDOM = [("dec-%d" % i, _random_member(i)) for i in range(400)]

# the constructive members, then the fixed strings (named, no stated class): what the slower device paths are shown
NAMED = [(name, b) for name, b, _ in CONSTRUCTIVE] + FIXED
# everything
CORPUS = NAMED + RANDOM


def is_valid(b32):
    return classify(b32) == "valid"
