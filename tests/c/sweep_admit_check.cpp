// sweep_admit_check.cpp — which state a general sweep owns (csrc/ksim_sweep_admit.h) under the system
// compiler, without a device: a stand-alone program with its own main (tests/test_sweep_plan_host.py
// compiles and runs it, once more under the address and undefined-behaviour sanitizers).  Every
// combination of the table facts and the entry is checked against the rule written out here a second
// time, as the entries' documents state it; then the named cases.  Prints "ok" or the failed checks.
#include <cstdio>

#include "ksim_sweep_admit.h"

namespace {

int failures = 0;

#define CHECK(cond)                                             \
  do {                                                          \
    if (!(cond)) {                                              \
      std::printf("line %d: %s\n", __LINE__, #cond);            \
      ++failures;                                               \
    }                                                           \
  } while (0)

constexpr int32_t MAXZ = 512;

// facts of a handle with nothing loaded, asked by ksim_sweep_nodes / ksim_sweep_drain
KsimSweepFacts none() {
  KsimSweepFacts f{};
  f.max_zones = MAXZ;
  return f;
}
KsimSweepFacts spread_tables(int32_t zones = 3) {  // SelectorSpread state alone
  KsimSweepFacts f = none();
  f.have_aff = true;
  f.n_zone = zones;
  f.any_spread = true;
  return f;
}
KsimSweepFacts term_tables(int32_t zones = 3, bool any_spread = false) {  // a required term in a pod class
  KsimSweepFacts f = spread_tables(zones);
  f.any_spread = any_spread;
  f.max_req = 1;
  return f;
}

// The instantiation family a sweep takes once the queue is known: queue_aff = a range or prefix pod has
// affinity or spread state.  'P' plain, 'S' SPR, 'I' IPA; 'x' = that pod is refused.  VOL goes on top (k.vol).
char family(const KsimSweepKind& k, bool queue_aff) {
  if (k.ipa) return 'I';
  if (!queue_aff) return 'P';
  return k.spread_bar == KSIM_SWEEP_SPREAD_OPEN ? 'S' : 'x';
}

void truth_table() {
  // every combination: 2 have_aff x 16 term counts x 2 launch tables x 3 zones x 2 spread x 2 have_vol x 5 entries
  const int32_t zones[3] = {0, MAXZ, MAXZ + 1};
  const bool entries[5][3] = {{false, false, false}, {true, false, false}, {false, true, false}, {false, false, true},
                              {true, true, false}};  // (ipa, vol, pol); the last one no entry sets, the rule still holds
  int n = 0;
  for (int bits = 0; bits < (1 << 9); ++bits)
    for (int32_t z : zones)
      for (auto& e : entries) {
        KsimSweepFacts f{};
        f.have_aff = bits & 1;
        f.n_carry = (bits >> 1) & 1; f.max_req = (bits >> 2) & 1; f.max_pref = (bits >> 3) & 1; f.max_car = ((bits >> 4) & 1) * 7;
        f.launch_tables = (bits >> 5) & 1;
        f.any_spread = (bits >> 6) & 1;
        f.have_vol = (bits >> 7) & 1;
        f.n_zone = z;
        f.max_zones = MAXZ;
        f.ipa = e[0]; f.vol = e[1]; f.pol = e[2];
        if (bits >> 8) f.max_zones = 0;  // no zone fits
        const KsimSweepKind k = ksim_sweep_admit_tables(f);
        ++n;
        const bool terms = f.have_aff && (f.n_carry || f.max_req || f.max_pref || f.max_car);
        const bool many = f.n_zone > f.max_zones;
        CHECK(k.terms == terms);
        // IPA: asked for, or terms in the tables under an entry that sweeps whatever the tables hold
        CHECK(k.ipa == (f.ipa || (terms && (f.vol || f.pol))));
        // VOL: asked for, or volume tables under the policy entry
        CHECK(k.vol == (f.vol || (f.pol && f.have_vol)));
        // refusals and their precedence: volume tables, affinity tables, zones
        KsimSweepRefusal want = KSIM_SWEEP_ADMITTED;
        if (f.vol && !f.have_vol) want = KSIM_SWEEP_NO_VOLUME_TABLES;
        else if (f.ipa && !f.have_aff) want = KSIM_SWEEP_NO_AFFINITY_TABLES;
        else if (k.ipa && many && f.any_spread) want = KSIM_SWEEP_AFFINITY_ZONES;
        CHECK(k.refusal == want);
        // spread state of a queue pod: barred only on tables whose terms are not swept, by terms first,
        // then launch tables, then zones
        KsimSweepSpreadBar bar = KSIM_SWEEP_SPREAD_OPEN;
        if (f.have_aff && !k.ipa) bar = terms ? KSIM_SWEEP_SPREAD_TERMS : f.launch_tables ? KSIM_SWEEP_SPREAD_LAUNCH_TABLES
                                                 : many ? KSIM_SWEEP_SPREAD_ZONES : KSIM_SWEEP_SPREAD_OPEN;
        CHECK(k.spread_bar == bar);
        // a sweep that owns the inter-pod terms never bars spread state; without tables nothing is barred
        if (k.ipa || !f.have_aff) CHECK(k.spread_bar == KSIM_SWEEP_SPREAD_OPEN);
        // only the affinity entry can be refused for missing affinity tables: the others take IPA from the tables
        if (!f.ipa) CHECK(k.refusal != KSIM_SWEEP_NO_AFFINITY_TABLES);
        if (f.pol && !f.vol) CHECK(k.refusal != KSIM_SWEEP_NO_VOLUME_TABLES);
      }
  CHECK(n == 512 * 3 * 5);
}

void named_cases() {
  KsimSweepKind k;
  // ksim_sweep_nodes / ksim_sweep_drain: plain without affinity state, SPR with it, on spread-only tables
  k = ksim_sweep_admit_tables(none());
  CHECK(!k.ipa && !k.vol && !k.refusal && family(k, false) == 'P' && family(k, true) == 'S');
  k = ksim_sweep_admit_tables(spread_tables());
  CHECK(!k.ipa && !k.vol && !k.refusal && family(k, false) == 'P' && family(k, true) == 'S');
  // ... and on tables with terms a plain queue is still swept, a pod with state refused for the terms
  k = ksim_sweep_admit_tables(term_tables());
  CHECK(!k.refusal && family(k, false) == 'P' && family(k, true) == 'x' && k.spread_bar == KSIM_SWEEP_SPREAD_TERMS);
  for (int which = 0; which < 4; ++which) {  // each term count alone makes terms
    KsimSweepFacts f = spread_tables();
    (which == 0 ? f.n_carry : which == 1 ? f.max_req : which == 2 ? f.max_pref : f.max_car) = 2;
    CHECK(ksim_sweep_admit_tables(f).spread_bar == KSIM_SWEEP_SPREAD_TERMS);
    f.have_aff = false;  // (counts left behind by tables no longer loaded are not terms)
    CHECK(!ksim_sweep_admit_tables(f).terms);
  }
  {  // launch tables, zones, and their order behind the terms
    KsimSweepFacts f = spread_tables(MAXZ + 1);
    CHECK(ksim_sweep_admit_tables(f).spread_bar == KSIM_SWEEP_SPREAD_ZONES);
    f.n_zone = MAXZ;
    CHECK(ksim_sweep_admit_tables(f).spread_bar == KSIM_SWEEP_SPREAD_OPEN);
    f.n_zone = MAXZ + 1;
    f.launch_tables = true;
    CHECK(ksim_sweep_admit_tables(f).spread_bar == KSIM_SWEEP_SPREAD_LAUNCH_TABLES);
    f.max_pref = 1;
    CHECK(ksim_sweep_admit_tables(f).spread_bar == KSIM_SWEEP_SPREAD_TERMS);
  }

  // ksim_sweep_affinity: IPA over every range; needs the tables; zones only with a spread pair
  KsimSweepFacts a = term_tables();
  a.ipa = true;
  k = ksim_sweep_admit_tables(a);
  CHECK(k.ipa && !k.vol && !k.refusal && family(k, false) == 'I' && family(k, true) == 'I');
  a = spread_tables();  // no terms: still IPA, the entry asks for it
  a.ipa = true;
  CHECK(ksim_sweep_admit_tables(a).ipa && !ksim_sweep_admit_tables(a).refusal);
  a = none();
  a.ipa = true;
  CHECK(ksim_sweep_admit_tables(a).refusal == KSIM_SWEEP_NO_AFFINITY_TABLES);
  a = term_tables(MAXZ + 1, false);
  a.ipa = true;
  CHECK(!ksim_sweep_admit_tables(a).refusal);
  a.any_spread = true;
  CHECK(ksim_sweep_admit_tables(a).refusal == KSIM_SWEEP_AFFINITY_ZONES);
  a.n_zone = MAXZ;
  CHECK(!ksim_sweep_admit_tables(a).refusal);
  a.launch_tables = true;  // (launch tables are the caller's refusal, for every range: not decided here)
  CHECK(!ksim_sweep_admit_tables(a).refusal && ksim_sweep_admit_tables(a).spread_bar == KSIM_SWEEP_SPREAD_OPEN);

  // ksim_sweep_volumes: needs volume tables (before anything about affinity); VOL on top of plain / SPR, or
  // of IPA when the tables hold terms
  KsimSweepFacts v = none();
  v.vol = true;
  CHECK(ksim_sweep_admit_tables(v).refusal == KSIM_SWEEP_NO_VOLUME_TABLES);
  v.have_vol = true;
  k = ksim_sweep_admit_tables(v);
  CHECK(k.vol && !k.ipa && !k.refusal && family(k, false) == 'P' && family(k, true) == 'S');
  v = spread_tables(MAXZ + 1);
  v.vol = v.have_vol = true;
  k = ksim_sweep_admit_tables(v);
  CHECK(k.vol && !k.ipa && !k.refusal && family(k, true) == 'x' && k.spread_bar == KSIM_SWEEP_SPREAD_ZONES);
  v = term_tables(MAXZ + 1, true);
  v.vol = v.have_vol = true;
  k = ksim_sweep_admit_tables(v);
  CHECK(k.vol && k.ipa && k.refusal == KSIM_SWEEP_AFFINITY_ZONES);
  v.have_vol = false;  // two apply: the volume tables are reported
  CHECK(ksim_sweep_admit_tables(v).refusal == KSIM_SWEEP_NO_VOLUME_TABLES);
  v = term_tables();
  v.vol = v.have_vol = true;
  k = ksim_sweep_admit_tables(v);
  CHECK(k.vol && k.ipa && !k.refusal && family(k, false) == 'I');
  v.ipa = true;  // (both asked, no tables of either: the volume tables first)
  v.have_vol = v.have_aff = false;
  CHECK(ksim_sweep_admit_tables(v).refusal == KSIM_SWEEP_NO_VOLUME_TABLES);
  v.have_vol = true;
  CHECK(ksim_sweep_admit_tables(v).refusal == KSIM_SWEEP_NO_AFFINITY_TABLES);

  // ksim_sweep_policy: never refused for missing tables; VOL follows the volume tables, IPA the terms
  KsimSweepFacts p = none();
  p.pol = true;
  k = ksim_sweep_admit_tables(p);
  CHECK(!k.vol && !k.ipa && !k.refusal && family(k, false) == 'P' && family(k, true) == 'S');
  p.have_vol = true;
  CHECK(ksim_sweep_admit_tables(p).vol && !ksim_sweep_admit_tables(p).refusal);
  p = term_tables();
  p.pol = true;
  k = ksim_sweep_admit_tables(p);
  CHECK(k.ipa && !k.vol && !k.refusal && k.spread_bar == KSIM_SWEEP_SPREAD_OPEN);
  p = spread_tables();
  p.pol = true;
  p.launch_tables = true;
  k = ksim_sweep_admit_tables(p);
  CHECK(!k.ipa && family(k, false) == 'P' && family(k, true) == 'x' && k.spread_bar == KSIM_SWEEP_SPREAD_LAUNCH_TABLES);
  p = term_tables(MAXZ + 1, true);
  p.pol = true;
  CHECK(ksim_sweep_admit_tables(p).refusal == KSIM_SWEEP_AFFINITY_ZONES);
}

}  // namespace

int main() {
  truth_table();
  named_cases();
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
