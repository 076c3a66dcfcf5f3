// polsweep_rules_check.cpp — the weight rules of ksim_sweep_policy (csrc/ksim_polsweep_rules.h) under
// the system compiler, without a device: a stand-alone program with its own main
// (tests/test_sweep_policy_host.py compiles and runs it).  Prints "ok" or the first failed check.
#include <cstdio>
#include <vector>

#include "ksim_polsweep_rules.h"

namespace {

int failures = 0;

#define CHECK(cond)                                             \
  do {                                                          \
    if (!(cond)) {                                              \
      std::printf("line %d: %s\n", __LINE__, #cond);            \
      ++failures;                                               \
    }                                                           \
  } while (0)

struct Verdict {
  KsimPolicyRule rule;
  int32_t scen;
  int slot;
};

Verdict run(const int64_t* hw, int no_prio, const std::vector<int64_t>& w, int bits = 27) {
  Verdict v{};
  v.rule = ksim_policy_weight_rules(hw, no_prio, w.data(), (int32_t)(w.size() / KSIM_NW), bits, &v.scen, &v.slot);
  return v;
}

// a row in slot order: LeastRequested, MostRequested, Balanced, TaintToleration, NodeAffinity, InterPod, Spread
std::vector<int64_t> rows(std::initializer_list<std::initializer_list<int64_t>> rs) {
  std::vector<int64_t> out;
  for (auto& r : rs) {
    CHECK(r.size() == KSIM_NW);
    out.insert(out.end(), r.begin(), r.end());
  }
  return out;
}

}  // namespace

int main() {
  static_assert(KSIM_W_LEAST_REQUESTED == 0 && KSIM_W_MOST_REQUESTED == 1 && KSIM_W_BALANCED == 2 &&
                    KSIM_W_TAINT_TOLERATION == 3 && KSIM_W_NODE_AFFINITY == 4 && KSIM_W_INTERPOD_AFFINITY == 5 &&
                    KSIM_W_SELECTOR_SPREAD == 6 && KSIM_NW == 7,
                "the rows below are written in slot order");
  const int64_t full[KSIM_NW] = {1, 0, 1, 1, 1, 1, 1};      // the default provider
  const int64_t stripped[KSIM_NW] = {1, 0, 1, 0, 0, 0, 0};  // map priorities only
  const int64_t wmax = ((int64_t)1 << 27) / 10 - 1;

  // the handle's own row, every restricted weight dropped, every one rescaled, the free slots at will
  CHECK(run(full, 0, rows({{1, 0, 1, 1, 1, 1, 1}})).rule == KSIM_POLICY_OK);
  CHECK(run(full, 0, rows({{1, 0, 1, 0, 0, 0, 0}, {0, 5, 0, 7, 9, 2, 3}, {0, 0, 0, 0, 0, 0, 1}})).rule == KSIM_POLICY_OK);
  CHECK(run(stripped, 0, rows({{0, 9, 4, 0, 0, 0, 0}, {3, 3, 3, 0, 0, 0, 0}})).rule == KSIM_POLICY_OK);
  // (an all-zero row passes here: the Python builder refuses an empty scenario)
  CHECK(run(full, 0, rows({{0, 0, 0, 0, 0, 0, 0}})).rule == KSIM_POLICY_OK);
  CHECK(run(full, 0, {}).rule == KSIM_POLICY_OK);

  // an empty prioritizer list in the handle: refused whatever the rows say
  CHECK(run(full, 1, rows({{1, 0, 1, 1, 1, 1, 1}})).rule == KSIM_POLICY_NO_PRIORITIES);

  // a negative weight, in any slot, names its scenario and slot
  for (int k = 0; k < KSIM_NW; ++k) {
    std::vector<int64_t> w = rows({{1, 0, 1, 1, 1, 1, 1}, {1, 0, 1, 1, 1, 1, 1}});
    w[KSIM_NW + k] = -1;
    const Verdict v = run(full, 0, w);
    CHECK(v.rule == KSIM_POLICY_RANGE && v.scen == 1 && v.slot == k);
  }

  // a restricted slot the handle's policy lacks: each of the four, alone; the free slots are never restricted
  for (int k : KSIM_POLICY_RESTRICTED_SLOTS) {
    std::vector<int64_t> w = rows({{1, 0, 1, 0, 0, 0, 0}, {1, 0, 1, 0, 0, 0, 0}, {1, 0, 1, 0, 0, 0, 0}});
    w[2 * KSIM_NW + k] = 1;
    const Verdict v = run(stripped, 0, w);
    CHECK(v.rule == KSIM_POLICY_RESTRICTED && v.scen == 2 && v.slot == k);
    int64_t one[KSIM_NW] = {1, 0, 1, 0, 0, 0, 0};
    one[k] = 4;  // ... and allowed, at any scale, as soon as the handle weighs it
    CHECK(run(one, 0, w).rule == KSIM_POLICY_OK);
  }
  {  // a handle with TaintToleration alone: NodeAffinity stays refused
    const int64_t tt[KSIM_NW] = {1, 0, 0, 2, 0, 0, 0};
    const Verdict v = run(tt, 0, rows({{1, 0, 0, 5, 0, 0, 0}, {1, 0, 0, 5, 1, 0, 0}}));
    CHECK(v.rule == KSIM_POLICY_RESTRICTED && v.scen == 1 && v.slot == KSIM_W_NODE_AFFINITY);
  }

  // the packed score: 10 x (LR + MR + BRA + spread + inter-pod) in 27 bits; TaintToleration and
  // NodeAffinity are not packed
  CHECK(run(full, 0, rows({{wmax, 0, 0, 0, 0, 0, 0}})).rule == KSIM_POLICY_OK);
  CHECK(run(full, 0, rows({{wmax - 4, 1, 1, 0, 0, 1, 1}})).rule == KSIM_POLICY_OK);
  CHECK(run(full, 0, rows({{1, 0, 1, wmax + 5, wmax + 5, 0, 0}})).rule == KSIM_POLICY_OK);
  {
    const Verdict v = run(full, 0, rows({{1, 0, 1, 1, 1, 1, 1}, {wmax - 3, 1, 1, 0, 0, 1, 1}}));
    CHECK(v.rule == KSIM_POLICY_SCORE && v.scen == 1);
  }
  for (int k : {KSIM_W_LEAST_REQUESTED, KSIM_W_MOST_REQUESTED, KSIM_W_BALANCED, KSIM_W_SELECTOR_SPREAD,
                KSIM_W_INTERPOD_AFFINITY}) {
    std::vector<int64_t> w = rows({{0, 0, 0, 0, 0, 0, 0}});
    w[k] = wmax + 1;
    CHECK(run(full, 0, w).rule == KSIM_POLICY_SCORE);
    w[k] = INT64_MAX;  // no overflow in the sum
    w[KSIM_W_LEAST_REQUESTED == k ? KSIM_W_BALANCED : KSIM_W_LEAST_REQUESTED] = INT64_MAX;
    CHECK(run(full, 0, w).rule == KSIM_POLICY_SCORE);
  }
  CHECK(run(full, 0, rows({{6, 0, 0, 0, 0, 0, 0}}), 6).rule == KSIM_POLICY_SCORE);  // 2^6 / 10 - 1 = 5
  CHECK(run(full, 0, rows({{5, 0, 0, 0, 0, 0, 0}}), 6).rule == KSIM_POLICY_OK);

  // the first broken rule in scenario order is the one reported
  {
    const Verdict v = run(stripped, 0, rows({{1, 0, 1, 0, 0, 0, 0}, {1, 0, 1, 1, 0, 0, 0}, {-1, 0, 0, 0, 0, 0, 0}}));
    CHECK(v.rule == KSIM_POLICY_RESTRICTED && v.scen == 1 && v.slot == KSIM_W_TAINT_TOLERATION);
  }
  for (int k = 0; k < KSIM_NW; ++k) CHECK(ksim_policy_slot_name(k)[0] != '?');

  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
