// ksim_sweep_admit.h — which per-scenario state a general sweep owns, decided from table facts alone
// (ksim_sweep_rt.cpp, admit): no device include and no handle, so that a host program can run the
// whole truth table (tests/c/sweep_admit_check.cpp).  The messages stay with the caller.
#pragma once
#include <stdint.h>

// What is loaded, and which entry asks.
struct KsimSweepFacts {
  bool have_aff;        // affinity tables are loaded ...
  int32_t n_carry, max_req, max_pref, max_car;  // ... their carried terms, and the most required / preferred /
                                                // carried terms of a pod class: any non-zero = inter-pod terms
  bool launch_tables;   // auxiliary spreading priority or CheckServiceAffinity lender tables are in force
  int32_t n_zone;       // zones of the affinity tables
  int32_t max_zones;    // ... and how many a swept SelectorSpread queue takes
  bool any_spread;      // an affinity class has a SelectorSpread pair
  bool have_vol;        // volume tables are loaded
  bool ipa, vol, pol;   // the entry: ksim_sweep_affinity, ksim_sweep_volumes, ksim_sweep_policy
};

// A table-level refusal of the whole call.
enum KsimSweepRefusal {
  KSIM_SWEEP_ADMITTED = 0,
  KSIM_SWEEP_NO_VOLUME_TABLES,    // ksim_sweep_volumes without volume tables
  KSIM_SWEEP_NO_AFFINITY_TABLES,  // ksim_sweep_affinity without affinity tables
  KSIM_SWEEP_AFFINITY_ZONES,      // inter-pod terms swept, a spread pair, and more zones than the kernel's LDS words
};

// Why a queue pod with affinity or spread state cannot be swept under SelectorSpread alone (the SPR
// instantiations).  Such a pod is then refused; a queue without one is swept all the same.
enum KsimSweepSpreadBar {
  KSIM_SWEEP_SPREAD_OPEN = 0,
  KSIM_SWEEP_SPREAD_TERMS,          // the tables hold inter-pod affinity terms
  KSIM_SWEEP_SPREAD_LAUNCH_TABLES,  // auxiliary spreading priority or lender tables
  KSIM_SWEEP_SPREAD_ZONES,          // more zones than a swept SelectorSpread queue takes
};

struct KsimSweepKind {
  bool terms;  // the tables hold inter-pod affinity terms
  bool ipa;    // every scenario owns carried terms and a raw column (the IPA instantiations, on top of SPR)
  bool vol;    // every scenario owns its mounts (the VOL instantiations)
  KsimSweepSpreadBar spread_bar;
  KsimSweepRefusal refusal;  // the first that applies, in the order of the enum
};

// ksim_sweep_affinity sweeps inter-pod terms over every range.  ksim_sweep_volumes and ksim_sweep_policy
// take the IPA instantiations when the tables hold such terms, and else the SPR or plain ones by the rule
// of every range; ksim_sweep_policy owns mounts when volume tables are loaded, ksim_sweep_volumes needs
// them.  With inter-pod terms swept the zones are refused only where a class has a spread pair (else
// the zone words stay unused), and nothing bars spread state.
inline KsimSweepKind ksim_sweep_admit_tables(const KsimSweepFacts& f) {
  KsimSweepKind k{};
  k.terms = f.have_aff && (f.n_carry || f.max_req || f.max_pref || f.max_car);
  k.ipa = f.ipa || ((f.vol || f.pol) && k.terms);
  k.vol = f.vol || (f.pol && f.have_vol);
  const bool zones = f.n_zone > f.max_zones;
  if (f.vol && !f.have_vol) k.refusal = KSIM_SWEEP_NO_VOLUME_TABLES;
  else if (k.ipa && !f.have_aff) k.refusal = KSIM_SWEEP_NO_AFFINITY_TABLES;
  else if (k.ipa && zones && f.any_spread) k.refusal = KSIM_SWEEP_AFFINITY_ZONES;
  if (f.have_aff && !k.ipa)
    k.spread_bar = k.terms ? KSIM_SWEEP_SPREAD_TERMS : f.launch_tables ? KSIM_SWEEP_SPREAD_LAUNCH_TABLES
                   : zones ? KSIM_SWEEP_SPREAD_ZONES : KSIM_SWEEP_SPREAD_OPEN;
  return k;
}
