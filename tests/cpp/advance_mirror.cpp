// The advancing forms of include/bpp.hpp from compiled code: a range proof inside a larger Fiat-Shamir protocol, as the reference's
// `&mut Transcript` allows it (src/range_proof.rs:222-237, :712-717).  Context is bound into a transcript, the proof is made and
// verified through the overloads that take their transcripts by pointer, and both sides go on with the same transcript.  The
// program checks what needs no oracle -- the const forms leave their arguments alone and give the same proof, the prover's state
// followed by r1, s1, d1 is the verifier's -- and prints the states and challenges, which tests/test_gpu_cpp_advance.py holds to
// the oracle.  Fixed inputs: n = 64, m = 1, extension degree 1, value 123456789, blinding factor 7, rng bytes i & 0xff.
#include <cstdio>
#include <cstdlib>

#include "bpp.hpp"

using namespace bpp_host;

#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      fprintf(stderr, "CHECK failed at line %d: %s\n", __LINE__, #x); \
      return 1;                                                   \
    }                                                             \
  } while (0)

static void hex(const char *name, const std::vector<uint8_t> &b) {
  printf("%s ", name);
  for (uint8_t x : b) printf("%02x", x);
  printf("\n");
}

int main() {
  Engine eng(0);
  auto params = RangeParameters::init(eng, 64, 1, create_pedersen_gens_with_extension_degree(ExtensionDegree::DefaultPedersen));
  Bytes32 blind{};
  blind[0] = 7;
  const uint64_t value = 123456789;
  const auto statement = RangeStatement::init(params, {params->commit(value, {blind})}, {std::nullopt}, std::nullopt);
  const auto witness = RangeWitness::init({CommitmentOpening::create(value, {blind})});
  std::vector<uint8_t> ext(32 * (6 + 3));
  for (size_t i = 0; i < ext.size(); i++) ext[i] = static_cast<uint8_t>(i);
  const std::vector<uint8_t> context{'b', 'l', 'o', 'c', 'k', ' ', '4', '2'};

  Transcript start = Transcript::create("outer protocol v1");
  start.append_message("context", context);
  start.append_u64("height", 42);
  const std::vector<uint8_t> state0 = start.state();
  CHECK(state0.size() == 203);

  // the const forms: same proof, arguments untouched
  const RangeProof plain = RangeProof::prove_with_rng(start, statement, witness, ext);
  CHECK(start.state() == state0);
  std::vector<Transcript> ts{start};
  CHECK(RangeProof::verify_batch(ts, {statement}, {plain}, VerifyAction::VerifyOnly).size() == 1);
  CHECK(ts[0].state() == state0);

  // the advancing forms
  Transcript tp = start;
  const RangeProof proof = RangeProof::prove_with_rng(&tp, statement, witness, ext);
  CHECK(proof == plain);
  CHECK(tp.state() != state0);
  const std::vector<uint8_t> prover_state = tp.state();
  std::vector<Transcript> tv{start};
  RangeProof::verify_batch(&tv, {statement}, {proof}, VerifyAction::VerifyOnly);
  const std::vector<uint8_t> verifier_state = tv[0].state();
  CHECK(verifier_state != prover_state && verifier_state != state0);
  std::vector<Transcript> tb{start};
  CHECK(RangeProof::prove_batch(&tb, {statement}, {witness}, {ext})[0] == plain && tb[0].state() == prover_state);

  // prover's state + r1, s1, d1 = verifier's state (wire format: [t] d1 A A1 B r1 s1 ...)
  const std::vector<uint8_t> &raw = proof.to_bytes();
  Transcript both = tp;
  both.append_message("r1", raw.data() + 1 + 32 + 96, 32);
  both.append_message("s1", raw.data() + 1 + 32 + 128, 32);
  both.append_message("d1", raw.data() + 1, 32);
  CHECK(both.state() == verifier_state);

  // a failed verification leaves the transcripts alone
  std::vector<uint8_t> bad = raw;
  bad[1 + 32 + 96] ^= 1;
  std::vector<Transcript> tf{start};
  bool threw = false;
  try {
    RangeProof::verify_batch(&tf, {statement}, {RangeProof::from_bytes(bad)}, VerifyAction::VerifyOnly);
  } catch (const ProofError &e) {
    threw = e.kind == ProofErrorKind::VerificationFailed;
  }
  CHECK(threw && tf[0].state() == state0);

  hex("proof", raw);
  hex("prover_state", prover_state);
  hex("verifier_state", verifier_state);
  hex("prover_after", tp.challenge_bytes("after", 32));
  hex("verifier_after", tv[0].challenge_bytes("after", 32));
  printf("advance_mirror ok\n");
  return 0;
}
