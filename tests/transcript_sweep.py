"""Test-side fixture: one proof for every position of the 166-byte STROBE block at which a caller's transcript can hand over.

Item L carries a transcript label of L bytes, L = 0 .. 165.  Transcript::new(label) leaves the sponge at position (28 + L) mod 166,
so the 166 labels are the 166 starting positions, and everything the range proof absorbs before its first challenge -- the domain
separator, H, G, N, T, M, the commitments, the promises, A, and the prover's cloned and re-keyed TranscriptRng -- is cut by the
block boundary at every possible place.  (After the first challenge the position is the same for every proof there is.)

Two shapes, both tiny (166 proofs of the C oracle's prover take a few seconds):
  A: n = 8, m = 1, t = 1, a seed nonce on every item, no promise: RecoverAndVerify, the masks are part of the comparison
  B: n = 4, m = 4, t = 3, a promise on every opening, no seed nonce: the 18-byte label of the promises, and a prover all of whose
     nonces come from a TranscriptRng cloned at the swept position

The items stand in the call in a fixed shuffled order (ORDER), so that neighbouring lanes and workgroups do not hold neighbouring
positions.  A shape is built once per process and never modified."""
import types

from oracle import cport
from oracle.pyref import merlin as M
from oracle.pyref import protocol as O
from tests.helpers import Prng, sb

RATE = M.STROBE_R  # 166
ORDER = [(61 * k + 17) % RATE for k in range(RATE)]  # call slot k holds label length ORDER[k]; 61 is coprime to 166
SHAPES = {"A": dict(n=8, m=1, t=1, seed_nonce=True, promise=False, action=1),
          "B": dict(n=4, m=4, t=3, seed_nonce=False, promise=True, action=0)}
_CACHE = {}


def label_of(length):
    """`length` deterministic, non-constant bytes"""
    return bytes((7 * i + length) & 0xff for i in range(length))


def start_state(length):
    """the 203 bytes of merlin::Transcript::new(label_of(length))"""
    return M.Transcript(label_of(length)).strobe.to_bytes()


def start_positions():
    """position of the sponge after Transcript::new, for label lengths 0 .. 165: 28, 29, .., 165, 0, .., 27"""
    return [start_state(length)[200] for length in range(RATE)]


class Sweep:
    """lengths / labels / states / positions: per call slot.  values, blindings, mins, seeds, ext: the witnesses and the external RNG
    bytes.  items: the C oracle's view of the batch (proof, commitments, promises, nonce, label).  masks, trace: what the C
    oracle's verify() returns for the whole batch as ONE reference batch."""

    def describe(self, k):
        return "shape %s, call slot %d: label of %d bytes, sponge handed over at position %d" % (self.name, k, self.lengths[k], self.positions[k])


def sweep(name):
    if name in _CACHE:
        return _CACHE[name]
    c = Sweep()
    c.name = name
    c.__dict__.update(SHAPES[name])
    c.rounds = (c.n * c.m).bit_length() - 1
    c.lengths = list(ORDER)
    c.labels = [label_of(length) for length in c.lengths]
    c.states = [start_state(length) for length in c.lengths]
    c.positions = [s[200] for s in c.states]
    rng = Prng(b"transcript-alignment-sweep-" + name.encode())
    cp = cport.Params(c.n, c.m, c.t)
    c.values, c.blindings, c.mins, c.seeds, c.ext, c.items = [], [], [], [], [], []
    top = (1 << c.n) - 1
    for k, label in enumerate(c.labels):
        values = [rng.next_u64() & top for _ in range(c.m)]  # the full range, top bit included
        if k < 2:
            values[0] = (top, 0)[k]  # and its two ends
        blindings = [[sb(O.random_not_zero(rng)) for _ in range(c.t)] for _ in range(c.m)]  # one of its own per generator
        mins = [(v // 3 if c.promise else None) for v in values]
        seed = sb(O.random_not_zero(rng)) if c.seed_nonce else None
        ext = rng.fill_bytes(32 * (c.rounds + 3))
        raw, comm = cp.prove(label, values, blindings, mins, seed, ext)
        c.values.append(values), c.blindings.append(blindings), c.mins.append(mins), c.seeds.append(seed), c.ext.append(ext)
        c.items.append({"proof": raw, "commitments": comm, "min_values": mins, "seed_nonce": seed, "label": label})
    rc, c.masks, c.trace = cp.verify(c.items, c.action, want_trace=True)
    cp.close()
    assert rc == 0, "the oracle rejects its own proofs (%d)" % rc
    if c.seed_nonce:
        assert c.masks == [b[0] for b in c.blindings]
    c.raw = [it["proof"] for it in c.items]
    c.commitments = [it["commitments"] for it in c.items]
    _CACHE[name] = c
    return c


def attach(c, bpp, engine):
    """the product's view of a sweep: parameters on `engine`, statements (with the nonces), witnesses, parsed proofs"""
    if getattr(c, "engine", None) is engine:
        return c
    c.engine = engine
    c.params = bpp.RangeParameters.init(c.n, c.m, bpp.create_pedersen_gens_with_extension_degree(c.t), engine=engine)
    c.statements = [bpp.RangeStatement.init(c.params, comm, mins, seed) for comm, mins, seed in zip(c.commitments, c.mins, c.seeds)]
    c.witnesses = [bpp.RangeWitness.init([bpp.CommitmentOpening.new(v, r) for v, r in zip(values, blindings)])
                   for values, blindings in zip(c.values, c.blindings)]
    c.proofs = [bpp.RangeProof.from_bytes(r) for r in c.raw]
    return c


def transcripts(bpp, c, how):
    """"labels": Transcript::new(label) per item; "states": the oracle's 203 bytes of the same transcripts"""
    if how == "labels":
        return [bpp.Transcript.new(label) for label in c.labels]
    return [bpp.Transcript.from_state(s) for s in c.states]


def trace_rows(c, trace):
    """the per-proof traces cut into one row per item: {name: [bytes per item]} (every item of a sweep has the same shape)"""
    widths = {"challenges": 32 * (c.rounds + 3), "rng_out": 32, "weights": 32, "dynamic_scalars": 32 * (c.m + 3 + 2 * c.rounds)}
    n = len(c.items)
    out = {}
    for name, w in widths.items():
        assert len(trace[name]) == n * w, (name, len(trace[name]), n * w)
        out[name] = [trace[name][k * w:(k + 1) * w] for k in range(n)]
    return out


TRACE_IDS = (("challenges", 1), ("rng_out", 2), ("weights", 3), ("static_scalars", 4), ("dynamic_scalars", 5))


def first_trace_difference(c, got):
    """got: {name: bytes} in the oracle's layout -> None, or a sentence naming the first item and the first trace that differ.
    The traces are looked at in the order in which a wrong sponge would spoil them."""
    want_rows, got_rows = trace_rows(c, c.trace), trace_rows(c, got)
    for name in ("challenges", "rng_out", "weights", "dynamic_scalars"):
        for k in range(len(c.items)):
            if got_rows[name][k] != want_rows[name][k]:
                bad = [j for j in range(len(c.items)) if got_rows[name][j] != want_rows[name][j]]
                return "%s: trace '%s' differs from the oracle's (%d of %d items differ, at label lengths %s)" % (
                    c.describe(k), name, len(bad), len(c.items), sorted(c.lengths[j] for j in bad)[:12])
    if got["static_scalars"] != c.trace["static_scalars"]:
        return "shape %s: trace 'static_scalars' (one row for the whole batch) differs from the oracle's" % c.name
    return None


def first_state_difference(c, got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        if g != w:
            bad = [j for j in range(len(want)) if got[j] != want[j]]
            return "%s: %s differs from the oracle's (%d of %d items differ, at label lengths %s)" % (
                c.describe(k), what, len(bad), len(want), sorted(c.lengths[j] for j in bad)[:12])
    return None if len(got) == len(want) else "%d rows for %d items" % (len(got), len(want))


def oracle_statement(c, k, o_params):
    """item k as the Python oracle's statement and witness (its prover advances a transcript in place; the C oracle's does not
    return one)"""
    openings = [O.CommitmentOpening(v, [int.from_bytes(r, "little") for r in rs]) for v, rs in zip(c.values[k], c.blindings[k])]
    comms = [o_params.pc_gens.commit(o.v, o.r) for o in openings]
    assert [p.compress() for p in comms] == c.commitments[k]
    seed = int.from_bytes(c.seeds[k], "little") if c.seeds[k] is not None else None
    return O.RangeStatement(o_params, comms, c.mins[k], seed), O.RangeWitness(openings)


def log_sponge(monkeypatch):
    """record what Strobe128 does from here on, without touching the oracle (only _absorb and _run_f are wrapped) -> a namespace:
    absorbs: [(length, position at entry)] of every _absorb, the two header bytes of an operation included;
    c_ops: [(the Strobe128 object, position after the header, absorbs so far)] of every operation with the C flag: at a position other than 0 its
           _begin_op permutes once more (forced), at 0 the header itself completed the block and it does not;
    run_f: [position] at every permutation"""
    log = types.SimpleNamespace(absorbs=[], c_ops=[], run_f=[])
    absorb, run_f = M.Strobe128._absorb, M.Strobe128._run_f

    def logged_absorb(self, data):
        # _begin_op sets pos_begin and cur_flags, then absorbs [old pos_begin, flags]: that is how a header is told from a message
        header = len(data) == 2 and self.pos_begin == self.pos + 1 and data[1] == self.cur_flags
        log.absorbs.append((len(data), self.pos))
        absorb(self, data)
        if header and data[1] & (M.FLAG_C | M.FLAG_K):
            log.c_ops.append((self, self.pos, len(log.absorbs)))

    def logged_run_f(self):
        log.run_f.append(self.pos)
        run_f(self)

    monkeypatch.setattr(M.Strobe128, "_absorb", logged_absorb)
    monkeypatch.setattr(M.Strobe128, "_run_f", logged_run_f)
    return log
