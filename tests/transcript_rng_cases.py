"""Test-side helpers of the transcript-protocol / transcript-RNG kinds of bpp_transcripts_enqueue: a program as plain tuples, run on
the oracle (oracle.pyref: merlin's builder call for call, protocol._challenge_scalar / _validate_and_append_point, curve.scalar_from_wide)
and on the library's host helpers, row by row.

A program is a list of
  ("append", label, [message of row i])      ("challenge", label, nbytes)
  ("point", label, [32 bytes of row i])      ("cscalar", label)
  ("begin",)  ("rekey", label, [witness of row i])  ("finalize", [32 bytes of row i] or None)
  ("fill", nbytes)  ("fill32", nbytes)  ("scalars", count)
Both runners return (states [n][203 bytes], outs: one list of n byte strings per output-writing op in program order, void: [bool]);
a void row (identity point, zero scalar) has state None."""
import ctypes

import numpy as np

from oracle.pyref import curve as C
from oracle.pyref import merlin as M
from oracle.pyref import protocol as O

WRITES = ("challenge", "cscalar", "fill", "fill32", "scalars")
L = C.L


def out_width(op):
    return {"challenge": lambda: op[2], "cscalar": lambda: 32, "fill": lambda: op[1], "fill32": lambda: op[1], "scalars": lambda: 32 * op[1]}[op[0]]()


def messages(seed, n, lengths):
    rng = np.random.default_rng(seed)
    return [bytes(rng.integers(0, 256, size=lengths[i], dtype=np.uint8)) for i in range(n)]


def sweep_makers():
    """the 169 rows of the existing sweep: every pos 0 .. 165 and labels of 166, 167 and 400 bytes"""
    from tests import transcript_sweep as TS
    makers = [(lambda k=k: M.Transcript(TS.label_of(k))) for k in list(range(166)) + [166, 167, 400]]
    assert sorted({mk().strobe.pos for mk in makers}) == list(range(166))
    return makers


def at(i, pos):
    """-> a function that makes row i's oracle transcript with the sponge at `pos`"""
    def make(length=None):
        tr = M.Transcript(b"row %d" % i)
        if length is None:
            length = (pos - make(0).strobe.pos) % 166
        tr.append_message(b"pad", bytes([i & 255]) * length)
        return tr
    assert make().strobe.pos == pos
    return make


def _scalar_bytes(v):
    return int(v).to_bytes(32, "little")


def oracle_rows(makers, prog, new=None):
    n = len(makers)
    states, void = [], []
    outs = [[] for op in prog if op[0] in WRITES]
    for i in range(n):
        tr = M.Transcript(new) if new is not None else makers[i]()
        builder = rng = None
        row_out = []
        try:
            for op in prog:
                kind = op[0]
                if kind == "append":
                    tr.append_message(op[1], op[2][i])
                elif kind == "challenge":
                    row_out.append(tr.challenge_bytes(op[1], op[2]))
                elif kind == "point":
                    O._validate_and_append_point(tr, op[1], op[2][i])
                elif kind == "cscalar":
                    row_out.append(_scalar_bytes(O._challenge_scalar(tr, op[1])))
                elif kind == "begin":
                    builder, rng = tr.build_rng(), None
                elif kind == "rekey":
                    builder = builder.rekey_with_witness_bytes(op[1], op[2][i])
                elif kind == "finalize":
                    rng = builder.finalize(M.NullRng() if op[1] is None else M.ByteStreamRng(op[1][i]))
                    builder = None
                elif kind == "fill":
                    row_out.append(rng.fill_bytes(op[1]))
                elif kind == "fill32":
                    row_out.append(b"".join(rng.fill_bytes(32) for _ in range(op[1] // 32)))
                elif kind == "scalars":
                    vals = [C.scalar_from_wide(rng.fill_bytes(64)) for _ in range(op[1])]
                    if any(v == 0 for v in vals):
                        raise O.ProofError(O.VERIFICATION_FAILED, "zero scalar")
                    row_out.append(b"".join(_scalar_bytes(v) for v in vals))
                else:
                    raise AssertionError(kind)
        except O.ProofError:
            states.append(None), void.append(True)
            for c, op in enumerate(o for o in prog if o[0] in WRITES):
                outs[c].append(bytes(out_width(op)))
            continue
        states.append(tr.strobe.to_bytes()), void.append(False)
        for c, b in enumerate(row_out):
            outs[c].append(b)
    return states, outs, void


def helper_rows(lib, start_states, prog):
    """the same program through bpp_transcript_* on host copies of the rows (start_states: [203 bytes])"""
    n = len(start_states)
    states, void = [], []
    outs = [[] for op in prog if op[0] in WRITES]
    buf = lambda b: (ctypes.c_uint8 * max(len(b), 1)).from_buffer_copy(bytes(b) or b"\0")  # noqa: E731
    for i in range(n):
        st = (ctypes.c_uint8 * 203).from_buffer_copy(start_states[i])
        rng = (ctypes.c_uint8 * 203)()
        err = ctypes.create_string_buffer(128)
        row_out, rc = [], 0
        for op in prog:
            kind = op[0]
            if kind == "append":
                rc = lib.bpp_transcript_append_message(st, buf(op[1]), len(op[1]), buf(op[2][i]), len(op[2][i]))
            elif kind == "challenge":
                o = (ctypes.c_uint8 * max(op[2], 1))()
                rc = lib.bpp_transcript_challenge_bytes(st, buf(op[1]), len(op[1]), o, op[2])
                row_out.append(bytes(o)[:op[2]])
            elif kind == "point":
                rc = lib.bpp_transcript_validate_and_append_point(st, buf(op[1]), len(op[1]), buf(op[2][i]), err, 128)
                if rc:
                    assert rc == O.VERIFICATION_FAILED and err.value == b"Identity element cannot be added to the transcript"
            elif kind == "cscalar":
                o = (ctypes.c_uint8 * 32)()
                rc = lib.bpp_transcript_challenge_scalar(st, buf(op[1]), len(op[1]), o, err, 128)
                row_out.append(bytes(o))
            elif kind == "begin":
                rc = lib.bpp_transcript_rng_begin(st, rng)
            elif kind == "rekey":
                rc = lib.bpp_transcript_rng_rekey(rng, buf(op[1]), len(op[1]), buf(op[2][i]), len(op[2][i]))
            elif kind == "finalize":
                rc = lib.bpp_transcript_rng_finalize(rng, None if op[1] is None else buf(op[1][i]))
            elif kind == "fill":
                o = (ctypes.c_uint8 * max(op[1], 1))()
                rc = lib.bpp_transcript_rng_fill(rng, o, op[1])
                row_out.append(bytes(o)[:op[1]])
            elif kind == "fill32":
                o = (ctypes.c_uint8 * 32)()
                got = b""
                for _ in range(op[1] // 32):
                    rc = rc or lib.bpp_transcript_rng_fill(rng, o, 32)
                    got += bytes(o)
                row_out.append(got)
            elif kind == "scalars":
                o = (ctypes.c_uint8 * 32)()
                got = b""
                for _ in range(op[1]):
                    rc = rc or lib.bpp_transcript_rng_scalar(rng, o, err, 128)
                    got += bytes(o)
                row_out.append(got)
            if rc:
                break
        if rc:
            states.append(None), void.append(True)
            for c, op in enumerate(o for o in prog if o[0] in WRITES):
                outs[c].append(bytes(out_width(op)))
            continue
        states.append(bytes(st)), void.append(False)
        for c, b in enumerate(row_out):
            outs[c].append(b)
    return states, outs, void


# ---- the programs both suites run (n rows each; seeds fixed)
def sweep_program(n):
    return [("begin",), ("rekey", b"w", messages(101, n, [32] * n)), ("finalize", messages(102, n, [32] * n)), ("fill", 32), ("scalars", 2),
            ("cscalar", b"e")]


L64 = bytes((3 * i + 1) & 0xFF for i in range(64))
WITNESS_LENS = (0, 1, 165, 166, 167, 400)
FILL_LENS = (0, 1, 165, 166, 167, 256, 257, 600)
SCALAR_COUNTS = (1, 4, 5, 9)


def edge_makers():
    return [at(k, (0, 1, 164, 165)[k % 4]) for k in range(12)]


def length_programs(n):
    """[(name, program, lens)]: lens True where the rekey's witnesses have per-row lengths under the cap 400"""
    progs = []
    for label in (b"", L64):
        for wl in WITNESS_LENS:
            progs.append(("witness %d label %d" % (wl, len(label)),
                          [("begin",), ("rekey", label, messages(200 + wl, n, [wl] * n)), ("finalize", messages(201, n, [32] * n)), ("fill", 32)], False))
    for shift in range(3):
        lens = [WITNESS_LENS[(k // 4 + k + shift) % 6] for k in range(n)]
        progs.append(("witness lens shift %d" % shift,
                      [("begin",), ("rekey", b"w", messages(210 + shift, n, lens)), ("finalize", None), ("fill32", 32)], True))
    for fl in FILL_LENS:
        progs.append(("fill %d" % fl, [("begin",), ("rekey", L64, messages(220, n, [32] * n)), ("finalize", messages(221, n, [32] * n)),
                                       ("fill", fl), ("fill", 7)], False))
    for f32 in (32, 13 * 32):
        progs.append(("fill32 %d" % f32, [("begin",), ("finalize", messages(230, n, [32] * n)), ("fill32", f32), ("fill", 5)], False))
    for count in SCALAR_COUNTS:
        progs.append(("scalars %d" % count, [("begin",), ("rekey", b"w", messages(240, n, [32] * n)), ("finalize", None), ("scalars", count),
                                             ("fill", 9)], False))
    return progs


def builder_programs(n):
    """[(name, program, new label or None)]: merlin's builder semantics"""
    w1, w2, e = messages(300, n, [32] * n), messages(301, n, [48] * n), messages(302, n, [32] * n)
    return [
        ("finalize without data is NullRng", [("begin",), ("rekey", b"w", w1), ("finalize", None), ("fill", 64)], None),
        ("two rekeys", [("begin",), ("rekey", b"w1", w1), ("rekey", b"w2", w2), ("finalize", e), ("fill", 64)], None),
        ("transcript ops between finalize and fill",
         [("begin",), ("rekey", b"w", w1), ("finalize", e), ("challenge", b"c", 32), ("append", b"a", w2), ("fill", 64)], None),
        ("the same without them", [("begin",), ("rekey", b"w", w1), ("finalize", e), ("fill", 64)], None),
        ("a second begin clones the advanced transcript",
         [("begin",), ("rekey", b"w", w1), ("append", b"a", w2), ("begin",), ("finalize", e), ("fill", 64)], None),
        ("fill32 of 64", [("begin",), ("finalize", e), ("fill32", 64)], None),
        ("fill of 64", [("begin",), ("finalize", e), ("fill", 64)], None),
        ("new then rng", [("begin",), ("rekey", b"w", w1), ("finalize", e), ("fill32", 64), ("scalars", 1)], b"fresh rows"),
    ]
