// ksim_polsweep_rules.h — the weight rules of ksim_sweep_policy (include/ksim_polsweep.h), free of
// any device include so that a host program can run them (tests/c/polsweep_rules_check.cpp).
#pragma once
#include <stdint.h>

#include "../../include/ksim.h"

// Why a scenario's weight row is refused.
enum KsimPolicyRule {
  KSIM_POLICY_OK = 0,
  KSIM_POLICY_NO_PRIORITIES,  // the handle has an empty prioritizer list
  KSIM_POLICY_RANGE,          // a negative weight
  KSIM_POLICY_RESTRICTED,     // a reduce, spread or inter-pod weight the handle's policy does not have
  KSIM_POLICY_SCORE,          // 10 x (the five packed weights) beyond the packed score
};

// The priorities whose tables exist only when the handle's own weight is non-zero.
static const int KSIM_POLICY_RESTRICTED_SLOTS[4] = {KSIM_W_TAINT_TOLERATION, KSIM_W_NODE_AFFINITY,
                                                    KSIM_W_INTERPOD_AFFINITY, KSIM_W_SELECTOR_SPREAD};

inline const char* ksim_policy_slot_name(int k) {
  switch (k) {
    case KSIM_W_LEAST_REQUESTED: return "LeastRequestedPriority";
    case KSIM_W_MOST_REQUESTED: return "MostRequestedPriority";
    case KSIM_W_BALANCED: return "BalancedResourceAllocation";
    case KSIM_W_TAINT_TOLERATION: return "TaintTolerationPriority";
    case KSIM_W_NODE_AFFINITY: return "NodeAffinityPriority";
    case KSIM_W_INTERPOD_AFFINITY: return "InterPodAffinityPriority";
    case KSIM_W_SELECTOR_SPREAD: return "SelectorSpreadPriority";
  }
  return "?";
}

// hw: the handle's KSIM_NW weights; w: [n_scen][KSIM_NW]; score_bits: the bits of the packed score.
// Returns the first rule broken, in scenario order, with the scenario in *scen and the slot (RANGE,
// RESTRICTED) in *slot.
inline KsimPolicyRule ksim_policy_weight_rules(const int64_t* hw, int no_prio, const int64_t* w, int32_t n_scen,
                                               int score_bits, int32_t* scen, int* slot) {
  *scen = 0;
  *slot = -1;
  if (no_prio) return KSIM_POLICY_NO_PRIORITIES;
  const int64_t wmax = ((int64_t)1 << score_bits) / 10 - 1;
  for (int32_t s = 0; s < n_scen; ++s) {
    const int64_t* row = w + (int64_t)s * KSIM_NW;
    *scen = s;
    for (int k = 0; k < KSIM_NW; ++k)
      if (row[k] < 0) {
        *slot = k;
        return KSIM_POLICY_RANGE;
      }
    for (int k : KSIM_POLICY_RESTRICTED_SLOTS)
      if (row[k] != 0 && hw[k] == 0) {
        *slot = k;
        return KSIM_POLICY_RESTRICTED;
      }
    int64_t tot = 0;  // each term is checked before it is added: no overflow
    for (int k : {KSIM_W_LEAST_REQUESTED, KSIM_W_MOST_REQUESTED, KSIM_W_BALANCED, KSIM_W_SELECTOR_SPREAD,
                  KSIM_W_INTERPOD_AFFINITY}) {
      if (row[k] > wmax) return KSIM_POLICY_SCORE;
      tot += row[k];
    }
    if (tot > wmax) return KSIM_POLICY_SCORE;
  }
  return KSIM_POLICY_OK;
}
