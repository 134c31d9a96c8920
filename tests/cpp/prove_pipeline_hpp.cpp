// Engine::prove_submit / prove_collect / prove_ticket_done of include/bpp.hpp in use (tests/test_prove_pipeline_host.py compiles this
// translation unit, syntax only: it needs no device and is never run).
#include "bpp.hpp"

using namespace bpp_host;

size_t outputs_from_a_queue(Engine &engine, uint64_t params, const std::vector<std::vector<bpp_prove_item>> &calls) {
  engine.prove_pipeline_depth(2);
  std::vector<Engine::ProveTicket> in_flight;
  size_t made = 0;
  auto take = [&](const Engine::ProveTicket &t) {
    const Engine::ProveResult r = engine.prove_collect(t);
    for (size_t i = 0; i < r.proofs.size(); i++) made += r.status[i] == 0 && !r.proofs[i].empty();
    if (t.openings) made += r.commitments.size();
    return r.code == 0 || !r.message.empty();
  };
  for (const auto &items : calls) {
    if (in_flight.size() == 2) {  // as many tickets outstanding as lanes
      take(in_flight.front());
      in_flight.erase(in_flight.begin());
    }
    in_flight.push_back(engine.prove_submit(params, items.data(), items.size()));
    in_flight.push_back(engine.prove_submit(params, items.data(), items.size(), true, 32 * 4));
    if (engine.prove_ticket_done(in_flight.back())) made++;
  }
  for (const auto &t : in_flight) take(t);
  return made + Engine::kProofStride;
}
