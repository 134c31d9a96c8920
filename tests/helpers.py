"""Test-side glue: builds the same batch for the product (bytes through the C ABI) and for the oracle (big ints).

Inputs follow the reference's own test recipe (tests/ristretto.rs:152-227, benches/range_proof.rs:206-262): value =
next_u64 % 2^(n-1), one random non-zero blinding repeated t times, seed nonce iff m == 1, transcript label
"BatchedRangeProofTest".  The PRNG is SHAKE256-based (the reference's ChaCha12 stream is not reproducible here and no
test of the reference depends on its actual bytes)."""
import contextlib
import hashlib
import types

from oracle.pyref import curve as C
from oracle.pyref import merlin as M
from oracle.pyref import protocol as O

LABEL = b"BatchedRangeProofTest"


class Prng:
    def __init__(self, seed):
        self._s = hashlib.shake_256(seed)
        self._off = 0

    def fill_bytes(self, n):
        out = self._s.digest(self._off + n)[self._off:]
        self._off += n
        return out

    def next_u64(self):
        return int.from_bytes(self.fill_bytes(8), "little")


def sb(x):
    return C.scalar_bytes(x)


class Case:
    pass


class _RecordingRng:
    """hands on another RNG's bytes and keeps them: the external RNG bytes of one oracle prove call, for the product's prover"""

    def __init__(self, rng):
        self._rng, self.taken = rng, b""

    def fill_bytes(self, n):
        out = self._rng.fill_bytes(n)
        self.taken += out
        return out


def oracle_pedersen_gens(extension_degree, h_base32, g_bases32):
    """the oracle's PedersenGens over caller-supplied bases (the reference's h_base / g_base_vec are public fields; the oracle's
    constructor only makes the default ones, so its four attributes are set here)"""
    assert len(g_bases32) == extension_degree
    pc = O.PedersenGens(extension_degree)
    pc.h_base, pc.h_base_compressed = C.decompress(h_base32), bytes(h_base32)
    pc.g_base_vec, pc.g_base_compressed_vec = [C.decompress(g) for g in g_bases32], [bytes(g) for g in g_bases32]
    assert pc.h_base is not None and all(g is not None for g in pc.g_base_vec)
    return pc


def custom_pedersen_gens(extension_degree, which="random", tag=b""):
    """"random": from_uniform_bytes of tagged SHAKE output; "edge" (t = 2): H = enc(4), G = [enc(6), enc(p - 3)], the smallest and
    the largest s that encode points"""
    if which == "edge":
        assert extension_degree == 2
        return oracle_pedersen_gens(2, (4).to_bytes(32, "little"), [(6).to_bytes(32, "little"), (C.P - 3).to_bytes(32, "little")])
    pts = [C.from_uniform_bytes(hashlib.shake_256(b"custom-base-%s-%d" % (tag, k)).digest(64)).compress()
           for k in range(extension_degree + 1)]
    return oracle_pedersen_gens(extension_degree, pts[0], pts[1:])


def make_oracle_batch(bit_length, aggregation, extension_degree, seed=b"8675309", strategy="third", m_max=None,
                      label=LABEL, pc_gens=None):
    """Oracle-side batch: parameters, statements, witnesses and proofs made by the oracle prover.  pc_gens: an oracle PedersenGens
    of the caller's own bases (oracle_pedersen_gens); with it every generator gets a blinding of its own."""
    rng = Prng(seed)
    c = Case()
    c.bit_length, c.aggregation, c.t = bit_length, list(aggregation), extension_degree
    c.label = label
    c.m_max = m_max or max(aggregation)
    c.pc_gens = pc_gens
    c.o_params = O.RangeParameters(bit_length, c.m_max, pc_gens if pc_gens is not None else O.PedersenGens(extension_degree))
    c.o_statements_private, c.o_statements_public, c.o_proofs, c.o_witnesses, c.expected_masks = [], [], [], [], []
    c.o_ext = []  # per proof: the bytes the oracle's prover drew from the external RNG, 32 per draw
    for m in aggregation:
        openings, commitments, mins = [], [], []
        for j in range(m):
            v = rng.next_u64() % (1 << (bit_length - 1))
            mins.append({"none": None, "third": v // 3, "eq": v}[strategy])
            if pc_gens is None:
                blind = [O.random_not_zero(rng)] * extension_degree
            else:
                blind = [O.random_not_zero(rng) for _ in range(extension_degree)]
            commitments.append(c.o_params.pc_gens.commit(v, blind))
            openings.append(O.CommitmentOpening(v, blind))
            if j == 0:
                c.expected_masks.append(list(blind) if m == 1 else None)
        w = O.RangeWitness(openings)
        sn = O.random_not_zero(rng) if m == 1 else None
        sp = O.RangeStatement(c.o_params, commitments, mins, sn)
        su = O.RangeStatement(c.o_params, commitments, mins, None)
        rec = _RecordingRng(rng)
        proof = O.prove_with_rng(M.Transcript(label), sp, w, rec)
        c.o_ext.append(rec.taken)
        c.o_statements_private.append(sp)
        c.o_statements_public.append(su)
        c.o_proofs.append(proof)
        c.o_witnesses.append(w)
    return c


def attach_product(c, pkg, eng):
    """Product-side view of an oracle batch: everything as bytes, bound to device parameters."""
    pc = c.pc_gens
    c.params = pkg.RangeParameters.init(c.bit_length, c.m_max, pkg.create_pedersen_gens_with_extension_degree(c.t) if pc is None
                                        else pkg.PedersenGens(c.t, pc.h_base_compressed, list(pc.g_base_compressed_vec)), engine=eng)
    c.statements_private, c.statements_public, c.proofs = [], [], []
    for sp in c.o_statements_private:
        comp = list(sp.commitments_compressed)
        c.statements_private.append(pkg.RangeStatement.init(c.params, comp, sp.minimum_value_promises,
                                                            sb(sp.seed_nonce) if sp.seed_nonce is not None else None))
        c.statements_public.append(pkg.RangeStatement.init(c.params, comp, sp.minimum_value_promises, None))
    for p in c.o_proofs:
        c.proofs.append(pkg.RangeProof.from_bytes(p.to_bytes()))
    c.transcripts = lambda: [pkg.Transcript.new(c.label) for _ in c.proofs]
    return c


def make_batch(pkg, eng, bit_length, aggregation, extension_degree, seed=b"8675309", strategy="third", m_max=None,
               label=LABEL, pc_gens=None):
    return attach_product(make_oracle_batch(bit_length, aggregation, extension_degree, seed, strategy, m_max, label, pc_gens),
                          pkg, eng)


def restate(c, o_params, private=False):
    """the oracle statements of batch c, bound to other parameters (same commitments, promises and nonces)"""
    return [O.RangeStatement(o_params, s.commitments, s.minimum_value_promises, s.seed_nonce if private else None)
            for s in c.o_statements_private]


def oracle_verify_trace(c, action=0, private=None, statements=None, proofs=None):
    """Run the oracle's verify() (no 256 cap) and return (masks as lists of 32-byte strings | None, trace)."""
    if statements is None:
        private = (action != 0) if private is None else private
        statements = c.o_statements_private if private else c.o_statements_public
    proofs = proofs if proofs is not None else c.o_proofs
    trace = {}
    masks = O.verify([M.Transcript(c.label) for _ in proofs], statements, proofs, action, trace=trace)
    out = [[sb(x) for x in m] if m is not None else None for m in masks]
    return out, trace


def trace_challenge_bytes(trace, max_rounds):
    """challenges in the layout of BPP_TRACE_CHALLENGES: per proof y, z, e_0.., e_final, zero padded to max_rounds+3"""
    out = b""
    for (y, z, rounds, e) in trace["challenges"]:
        row = [y, z] + list(rounds) + [e]
        row += [0] * (max_rounds + 3 - len(row))
        out += b"".join(sb(x) for x in row)
    return out


def replay_verifier_state(tr, n_bits, t, pc, commitments, mins, raw):
    """PASS 1 of the oracle's verify() (oracle/pyref/protocol.py: the loop at the head of verify) on `tr`, without the arithmetic
    behind it: what verify() leaves in the transcript of a proof"""
    proof = O.RangeProof.from_bytes(raw)
    st = types.SimpleNamespace(commitments_compressed=list(commitments), minimum_value_promises=list(mins))
    rpt = O.RangeProofTranscript(tr, pc.h_base_compressed, pc.g_base_compressed_vec, n_bits, t, len(commitments), st, None, M.NullRng())
    rpt.challenges_y_z(proof.a)
    for l, r in zip(proof.li, proof.ri):
        rpt.challenge_round_e(l, r)
    rpt.challenge_final_e(proof.a1, proof.b)
    rpt.to_verifier_rng(proof.r1, proof.s1, proof.d1)
    return tr.strobe.to_bytes()


# ---------------------------------------------------------------------------------------------------------------------------
# Chosen challenges (tests/test_verify_edges_host.py checks the families on the oracle, tests/test_gpu_verify_edges.py runs them
# through bpp_verify_batch_with_challenges).  The protocol is complete for ANY non-zero challenges (and y != 1): an
# honest prover run under forced challenges gives a proof that verifies under the same challenges exactly when every scalar of
# the verifier's PASS 2 and every MSM scalar is right.
MONT_R = 1 << 261  # csrc/scalar.h: nine 29-bit limbs


def mont_preimage(v):
    """the x whose Montgomery form x * 2^261 mod l is v"""
    return v * pow(MONT_R, -1, C.L) % C.L


# the ten values of the CPU experiment first (EDGE_SCALARS[:10]), then the limb-boundary ones
EDGE_SCALARS = [
    ("1", 1), ("2", 2), ("l-1", C.L - 1), ("l-2", C.L - 2), ("2^252", 1 << 252), ("(l+1)/2", (C.L + 1) // 2),
    ("mont^-1(1)", mont_preimage(1)), ("mont^-1(l-1)", mont_preimage(C.L - 1)), ("mont^-1(2^252-1)", mont_preimage((1 << 252) - 1)),
    ("mont^-1(2^252)", mont_preimage(1 << 252)),
    ("(l-1)/2", (C.L - 1) // 2), ("2^29-1", (1 << 29) - 1), ("2^29", 1 << 29), ("2^58", 1 << 58), ("2^232-1", (1 << 232) - 1),
    ("mont^-1(l-2)", mont_preimage(C.L - 2)), ("mont^-1(2^29-1)", mont_preimage((1 << 29) - 1)),
]
# name -> the image the entry claims under x -> x * 2^261 mod l
EDGE_MONT_IMAGES = {"mont^-1(1)": 1, "mont^-1(l-1)": C.L - 1, "mont^-1(2^252-1)": (1 << 252) - 1, "mont^-1(2^252)": 1 << 252,
                    "mont^-1(l-2)": C.L - 2, "mont^-1(2^29-1)": (1 << 29) - 1}


class ForcedRecord:
    """what the patched _challenge_scalar returned, one list per proof: [y, z, e_0.., e_final]"""

    def __init__(self):
        self.returned = []


@contextlib.contextmanager
def forced_challenges(rows):
    """Inside the block O._challenge_scalar still squeezes the transcript (so every later challenge, the transcript RNG and the
    verifier's weights stay functions of the proof) but returns rows[i][k] for challenge k of the i-th proof that passes through
    it, where that entry is not None.  A proof starts at its `y`; proofs past the end of `rows` keep their hashed values.  Yields
    a ForcedRecord; the original function is back on exit."""
    rows = [list(r) if r is not None else None for r in rows]
    assert all(v is None or 0 < v < C.L for r in rows if r is not None for v in r)
    orig, rec = O._challenge_scalar, ForcedRecord()

    def patched(t, label):
        v = orig(t, label)
        if label == b"y":
            rec.returned.append([])
        i, k = len(rec.returned) - 1, len(rec.returned[-1])
        if i < len(rows) and rows[i] is not None:
            assert k < len(rows[i]), "row %d is shorter than the proof's challenges" % i
            if rows[i][k] is not None:
                v = rows[i][k]
        rec.returned[-1].append(v)
        return v

    O._challenge_scalar = patched
    try:
        yield rec
    finally:
        O._challenge_scalar = orig


def oracle_verify_forced(c, row, action, private=None):
    """the oracle's verify() of case c's proof with the challenges of `row` -> (masks as bytes | None, ProofError | None, trace)"""
    private = (action != 0) if private is None else private
    trace = {}
    with forced_challenges([row]):
        try:
            masks = O.verify([M.Transcript(c.label)], [c.o_statement_private if private else c.o_statement_public], [c.o_proof],
                             action, trace=trace)
        except O.ProofError as e:
            return None, e, trace
    return [[sb(x) for x in m] if m is not None else None for m in masks], None, trace


def edge_challenge_case(n, m, t, row, seed, m_max=None, name=None):
    """One statement, witness and oracle proof made under the forced `row` ([y, z, e_0.., e_final], None = hashed), and what
    verify_batch_with_challenges needs to check it: c.challenges (one list of 32-byte scalars: the values the oracle's verifier
    was handed), c.rng_outputs (from the oracle's trace), c.expected_masks (the oracle's, under RecoverAndVerify for m == 1 and
    VerifyOnly otherwise) and the oracle objects.  The oracle's own verdict under the row is c.oracle_error (None: accepted)."""
    rounds = (n * m).bit_length() - 1
    assert len(row) == rounds + 3
    rng = Prng(seed)
    c = Case()
    c.name = name or "row"
    c.bit_length, c.m, c.t, c.m_max, c.label, c.row = n, m, t, m_max or m, LABEL, list(row)
    c.o_params = O.RangeParameters(n, c.m_max, O.PedersenGens(t))
    openings, commitments, mins = [], [], []
    for _ in range(m):
        v = rng.next_u64() % (1 << (n - 1))
        blind = [O.random_not_zero(rng) for _ in range(t)]
        mins.append(v // 3)
        commitments.append(c.o_params.pc_gens.commit(v, blind))
        openings.append(O.CommitmentOpening(v, blind))
    c.o_witness = O.RangeWitness(openings)
    sn = O.random_not_zero(rng) if m == 1 else None
    c.o_statement_private = O.RangeStatement(c.o_params, commitments, mins, sn)
    c.o_statement_public = O.RangeStatement(c.o_params, commitments, mins, None)
    with forced_challenges([row]) as made:
        c.o_proof = O.prove_with_rng(M.Transcript(c.label), c.o_statement_private, c.o_witness, rng)
    c.action = 1 if m == 1 else 0
    with forced_challenges([row]) as seen:
        trace = {}
        try:
            masks = O.verify([M.Transcript(c.label)], [c.o_statement_private if m == 1 else c.o_statement_public], [c.o_proof],
                             c.action, trace=trace)
            c.oracle_error = None
            c.expected_masks = [[sb(x) for x in mk] if mk is not None else None for mk in masks]
        except O.ProofError as e:
            c.oracle_error, c.expected_masks = e, None
    assert seen.returned == made.returned and len(seen.returned[0]) == len(row)
    assert all(f is None or f == v for f, v in zip(row, seen.returned[0]))
    c.values = list(seen.returned[0])  # every position, forced or hashed
    c.challenges = [[sb(v) for v in c.values]]
    c.rng_outputs = list(trace["rng_outputs"])
    c.witness_masks = [[sb(x) for x in openings[0].r]] if m == 1 else [None]
    return c


EDGE_POSITION_CLASSES = ("y", "z", "e_all", "e_first", "e_last", "e_final")


def _edge_rows(rounds):
    """(family, case name, row) for every family of a proof with `rounds` rounds"""
    width = rounds + 3
    where = {"y": [0], "z": [1], "e_all": list(range(2, 2 + rounds)), "e_first": [2], "e_last": [1 + rounds], "e_final": [2 + rounds]}
    for cls in EDGE_POSITION_CLASSES:
        for vname, v in EDGE_SCALARS:
            if cls == "y" and v == 1:
                continue  # the one non-zero challenge the verifier is not complete for (edge_y_one_case)
            row = [None] * width
            for k in where[cls]:
                row[k] = v
            yield cls, "%s=%s" % (cls, vname), row
    yield "all_edge", "all=l-1", [C.L - 1] * width
    # y sits at an even index: it gets l-1, never the excluded 1
    yield "all_edge", "alternating", [(C.L - 1, 1)[k & 1] for k in range(width)]


_EDGE_CACHE = {}


def edge_challenge_families(n, m, t, m_max=None, seed=b"edge", only=None):
    """{family: [cases]}: one case per (position class, edge value) -- y, z, every e_j, the first e_j alone, the last e_j alone,
    e_final -- and the family "all_edge" of two rows: every position l-1, and positions alternating l-1, 1 (its second case).
    `only`: the families to make (the others are left out of the dict).  Proving in Python is the cost, so the cases of a
    (shape, seed) are made once per process and shared by every test that asks; nobody changes them."""
    key = (n, m, t, m_max, seed)
    made = _EDGE_CACHE.setdefault(key, {})
    rounds = (n * m).bit_length() - 1
    out = {}
    for i, (fam, name, row) in enumerate(_edge_rows(rounds)):
        if only is not None and fam not in only:
            continue
        if name not in made:
            made[name] = edge_challenge_case(n, m, t, row, seed + b"-%d" % i, m_max, name)
        out.setdefault(fam, []).append(made[name])
    return out


def edge_y_one_case(n, m, t, seed=b"edge-y1"):
    """a proof made under y = 1"""
    rounds = (n * m).bit_length() - 1
    return edge_challenge_case(n, m, t, [1] + [None] * (rounds + 2), seed, name="y=1")


# ---------------------------------------------------------------------------------------------------------------------------
# Structured inputs of the bucket MSM (tests/test_gpu_msm_structured.py runs them on the device, tests/test_host_arith.py checks
# that each family still has the property it exists for).  A case is n terms: scalar i goes with bases[pidx[i]].  Few distinct
# bases, so that the oracle's answer is one short multiscalar multiplication over the scalars folded per base.
class MsmCase:
    def __init__(self, name, scalars, pidx, bases):
        assert len(scalars) == len(pidx) and all(0 <= s < C.L for s in scalars)
        self.name, self.scalars, self.pidx, self.bases = name, scalars, pidx, bases

    def __len__(self):
        return len(self.scalars)

    def folded(self):
        """one scalar per base: the sum of its terms' scalars mod l"""
        acc = [0] * len(self.bases)
        for s, p in zip(self.scalars, self.pidx):
            acc[p] += s
        return [a % C.L for a in acc]

    def expected(self):
        return C.multiscalar_mul(self.folded(), self.bases).compress()


_MSM_BASES = []


def msm_bases():
    """D = 7 distinct points, then their negatives (7..13), then the identity (14)"""
    if not _MSM_BASES:
        pts = [C.from_uniform_bytes(hashlib.shake_256(b"structured-p-%d" % i).digest(64)) for i in range(7)]
        _MSM_BASES.extend(pts + [-p for p in pts] + [C.Point.identity()])
    return _MSM_BASES


MSM_NEG, MSM_IDENT = 7, 14


def msm_hashed(tag, i, bits=253):
    """a hashed scalar below 2^bits, canonical"""
    return (int.from_bytes(hashlib.shake_256(b"structured-s-%s-%d" % (tag, i)).digest(32), "little") & ((1 << bits) - 1)) % C.L


MSM_CONSTANTS = [("hashed", msm_hashed(b"const", 0)), ("one", 1), ("l-1", C.L - 1), ("2^252", 1 << 252)]
MSM_TOP = [C.L - 1, C.L - 2, 1 << 252, (1 << 252) - 1, (1 << 252) + 1]
# low four bits 0011: window 0 of this scalar is never the bucket of digit +-1, whatever the window width
MSM_NOT_ONE = (msm_hashed(b"not-one", 0) & ~15) | 3


def _case(name, scalars, pidx=None):
    n = len(scalars)
    return MsmCase(name, list(scalars), list(pidx) if pidx is not None else [i % 7 for i in range(n)], msm_bases())


def msm_constant(n, s, name="constant"):
    """one scalar for every term: every window holds ONE bucket, of n terms"""
    return _case("%s-%d" % (name, n), [s] * n)


def msm_prefix(n, m, s, name):
    """m terms of one scalar, the other n - m terms zero (a zero has no digit: it lands in no bucket): bucket lists of exactly m"""
    assert m <= n
    return _case("%s-%d-of-%d" % (name, m, n), [s] * m + [0] * (n - m))


def msm_cancel(n, s, m=None):
    """P, -P alternating IN THE CALL as two encodings under one scalar (m terms, the rest zero): the identity for even m, sP for odd
    m.  The order inside a bucket's list is not the call's: k_msm_prelude scatters with atomics.  Whatever it is, every list holds
    as many P as -P (or one more P), so some prefix sum of it is the identity and, for m >= 4, some addition a doubling or a
    cancellation; WHERE in the list is not fixed."""
    m = n if m is None else m
    return _case("cancel-pm-%d-of-%d" % (m, n), [s] * m + [0] * (n - m), [(0, MSM_NEG)[i & 1] for i in range(n)])


def msm_cancel3(n, s):
    """P, P, -P repeating"""
    return _case("cancel-ppm-%d" % n, [s] * n, [(0, 0, MSM_NEG)[i % 3] for i in range(n)])


def msm_same_point(n, s):
    """D = 1: the second addition of every bucket is a doubling"""
    return _case("same-point-%d" % n, [s] * n, [0] * n)


def msm_identity_terms(n, where):
    """the encoding bytes(32) as a term: "first" / "middle" (its place IN THE CALL), "alone" (the only term of its bucket in window 0)
    or "all".  "first" and "middle" do not fix its place in the bucket's list -- k_msm_prelude scatters with atomics, the order
    inside a bucket is not the call's -- so the identity as the start of an accumulator (ge_from_niels_first) is likely there, not
    certain; "alone" and "all" guarantee it."""
    if where == "all":
        return _case("identity-all-%d" % n, [msm_hashed(b"ident", i) for i in range(n)], [MSM_IDENT] * n)
    at = {"first": 0, "middle": n // 2, "alone": n // 2}[where]
    scalars = [MSM_NOT_ONE] * n
    pidx = [i % 7 for i in range(n)]
    pidx[at] = MSM_IDENT
    if where == "alone":
        scalars[at] = 1
    return _case("identity-%s-%d" % (where, n), scalars, pidx)


def msm_small(n, bits):
    """every scalar below 2^bits: the windows above are empty"""
    return _case("small-%d-%d" % (bits, n), [msm_hashed(b"small%d" % bits, i, bits) for i in range(n)])


def msm_sparse(n, at):
    """all zero except term `at`"""
    scalars = [0] * n
    scalars[at] = msm_hashed(b"sparse", at) | 1
    return _case("sparse-%d-of-%d" % (at, n), scalars)


def msm_zero(n):
    return _case("zero-%d" % n, [0] * n)


def msm_ramp(n, shift=0):
    """s_i = (i + 1) << shift: shift 0 hits every bucket of the low window in turn, shift 120 a window that straddles a word"""
    return _case("ramp-%d-%d" % (shift, n), [(i + 1) << shift for i in range(n)])


def msm_window_widths(c):
    """the MSM's windows for width c (recode.h: msm_make_plan): K = ceil(253 / c) windows, the first K_wide of c bits, the others c - 1"""
    K = -(-253 // c)
    K_wide = 253 - K * (c - 1)
    return [c] * K_wide + [c - 1] * (K - K_wide)


def msm_half_chains(c):
    """the chain constructions of test_host_arith.py::test_scalar_recodings for window width c: nine windows whose raw value is
    exactly half their range -- alone (digits +half), with a carry coming in at the bottom, and starting one and two windows up.
    Built on the plan's own window boundaries (at c = 14 only six windows have 14 bits), which for c <= 13 are multiples of c."""
    wid = msm_window_widths(c)
    top = [sum(wid[:k + 1]) - 1 for k in range(len(wid))]  # the top bit of every window

    def chain(first):
        return sum(1 << top[k] for k in range(first, first + 9))
    return [x % C.L for x in (chain(0), chain(0) + (1 << (c - 1)) - 1, chain(1) + (1 << (c - 1)) + 1, chain(2) + (1 << c) - 1)]


def msm_chains(n, c):
    """the half-digit chains of width c first, hashed scalars after them"""
    ch = msm_half_chains(c)[:n]
    return _case("chains-c%d-%d" % (c, n), ch + [msm_hashed(b"chain-fill", i) for i in range(n - len(ch))])


def msm_top(n):
    return _case("top-%d" % n, [MSM_TOP[i % 5] for i in range(n)])


def msm_skew(n):
    """nine terms of ten share one scalar, the tenth is hashed: one huge bucket per window beside buckets of a few terms"""
    s = MSM_CONSTANTS[0][1]
    return _case("skew-%d" % n, [msm_hashed(b"skew", i) if i % 10 == 9 else s for i in range(n)])


# where the digit cache of k_msm_prelude ends at c = 13, 12, 11 (csrc/msm.h: msm_prelude_dig_cap; at c = 14 nothing is cached)
MSM_DIG_CAPS = {11: 24576, 12: 20480, 13: 12288, 14: 0}


def msm_structured_cases(n, c):
    """every family at n terms (families with a size of their own are padded with zero scalars, which reach no bucket)"""
    s = MSM_CONSTANTS[0][1]
    out = [msm_constant(n, v, "constant-" + tag) for tag, v in MSM_CONSTANTS]
    out += [msm_prefix(n, m, s, "clamp") for m in (254, 255, 256, 257) if m <= n]
    out += [msm_prefix(n, m, s, "pipeline") for m in range(1, 10) if m <= n]
    out += [msm_cancel(n, s), msm_cancel(n, s, n - 1), msm_cancel3(n, s), msm_same_point(n, s)]
    out += [msm_identity_terms(n, w) for w in ("first", "middle", "alone", "all")]
    out += [msm_small(n, 16), msm_small(n, 64)]
    out += [msm_sparse(n, at) for at in sorted({0, n - 1} | {e for cap in MSM_DIG_CAPS.values() for e in (cap - 1, cap) if 0 < e < n - 1})]
    out += [msm_zero(n), msm_ramp(n), msm_ramp(n, 120), msm_chains(n, c), msm_top(n), msm_skew(n)]
    assert all(len(x) == n for x in out)
    return out
