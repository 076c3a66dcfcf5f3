// Stand-alone check of csrc/ksim_sweep_plan.h (tests/test_sweep_plan_host.py compiles and runs it):
// the carver over layouts shaped like the sweep's three forms, and the chunk rule.  No device, no
// libksim: the element types below only stand in for the kernels' structs by size.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "ksim_sweep_plan.h"

namespace {

int failures = 0;
#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      ++failures;                              \
      printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      printf(__VA_ARGS__);                     \
      printf("\n");                            \
    }                                          \
  } while (0)

struct Ctx { char b[1864]; };    // a scenario's context
struct Aff { char b[328]; };     // its affinity descriptor
struct EvCfg { char b[40]; };    // its map weights, tree form
struct FPod { char b[48]; };     // a pod, scan form
constexpr size_t NREASONS = 13;  // words of a FitError histogram

struct Shape {
  const char* label;
  size_t N, P, S, T, NS, NP, aw, wcap, CL, K, leaves, levels;
  bool weights, absent, rq, spr;
};

// The carver, with every hand-out written down.
struct Arr { std::string name; uintptr_t p; size_t bytes; };
struct Rec {
  KsimSweepCarver& cv;
  std::vector<Arr> arrs;
  explicit Rec(KsimSweepCarver& c) : cv(c) {}
  template <class T>
  void take(const char* name, size_t count) {
    const size_t before = cv.bytes();
    T* p = cv.take<T>(count);
    arrs.push_back({name, reinterpret_cast<uintptr_t>(p), count * sizeof(T)});
    if (!count) CHECK(cv.bytes() == before, "%s: an empty array advanced the carver", name);
  }
};

void outputs(Rec& r, size_t C, const Shape& s) {
  r.take<int32_t>("out_node", C * s.P);
  r.take<uint64_t>("out_counter", C);
  if (s.absent) r.take<uint32_t>("absent", C * s.aw);
  if (s.wcap) {
    r.take<int32_t>("why_pod", C * s.wcap);
    r.take<int32_t>("why_hist", C * s.wcap * NREASONS);
  }
}

void general(Rec& r, size_t C, const Shape& s) {
  for (const char* col : {"req_cpu", "req_mem", "req_gpu", "req_eph", "nz_cpu", "nz_mem"}) r.take<int64_t>(col, C * s.N);
  for (const char* col : {"pod_count", "port_count", "flags"}) r.take<int32_t>(col, C * s.N);
  r.take<int64_t>("req_scalar", C * s.N * s.NS);
  r.take<uint64_t>("ports", C * s.N * s.NP);
  r.take<Ctx>("ctx", C);
  if (s.weights) r.take<int64_t>("w", s.S * 3);
  r.take<int32_t>("err", 1);
  outputs(r, C, s);
  if (s.rq) {
    r.take<int64_t>("off", s.S + 1);
    r.take<int64_t>("pod", s.T);
    r.take<int32_t>("out_pre", s.T);
  }
  if (s.spr) {
    r.take<int32_t>("cnt", C * s.CL);
    r.take<Aff>("aff", C);
  }
}

void scan(Rec& r, size_t C, const Shape& s) {
  for (const char* col : {"rc", "rm", "zc", "zm"}) r.take<double>(col, C * s.N);
  r.take<int32_t>("count", C * s.N);
  r.take<FPod>("pods", s.P);
  r.take<int32_t>("w", s.S * 3);
  outputs(r, C, s);
}

void tree(Rec& r, size_t C, const Shape& s) {
  for (const char* col : {"rc", "rm", "zc", "zm"}) r.take<int64_t>(col, C * s.N);
  r.take<int32_t>("count", C * s.N);
  r.take<int32_t>("leaves", C * s.K * s.leaves);
  r.take<uint64_t>("levels", C * s.levels);
  r.take<int32_t>("fitc", C * s.K);
  r.take<EvCfg>("cfg", C);
  outputs(r, C, s);
  r.take<char>("spare", 4096);
}

using Form = void (*)(Rec&, size_t, const Shape&);

void check_layout(const char* form, Form f, const Shape& s, size_t C) {
  auto layout = [&](KsimSweepCarver& cv, size_t c) {
    Rec r(cv);
    f(r, c, s);
  };
  const size_t need = ksim_sweep_measure(layout, C);  // as the runtime measures
  KsimSweepCarver mcv;  // the same pass over a null base, its offsets kept
  Rec m(mcv);
  f(m, C, s);
  CHECK(mcv.bytes() == need, "%s/%s C=%zu: two measuring passes disagree", form, s.label, C);
  CHECK(need % KsimSweepCarver::ALIGN == 0, "%s/%s: the size is not a multiple of the alignment", form, s.label);
  char* buf = static_cast<char*>(aligned_alloc(KsimSweepCarver::ALIGN, need ? need : KsimSweepCarver::ALIGN));
  KsimSweepCarver cv(buf);
  Rec r(cv);
  f(r, C, s);
  const uintptr_t lo = reinterpret_cast<uintptr_t>(buf), hi = lo + need;
  CHECK(r.cv.bytes() == need, "%s/%s C=%zu: measured %zu bytes, carved %zu", form, s.label, C, need, r.cv.bytes());
  CHECK(r.arrs.size() == m.arrs.size(), "%s/%s: the passes hand out different arrays", form, s.label);
  for (size_t i = 0; i < r.arrs.size(); ++i) {
    const Arr& a = r.arrs[i];
    CHECK(a.p % KsimSweepCarver::ALIGN == 0, "%s/%s: %s is not 256-byte aligned", form, s.label, a.name.c_str());
    CHECK(a.p >= lo && a.p + a.bytes <= hi, "%s/%s: %s leaves the buffer", form, s.label, a.name.c_str());
    CHECK(a.p - lo == m.arrs[i].p, "%s/%s: %s measured at another offset", form, s.label, a.name.c_str());
    for (size_t j = 0; j < i; ++j) {
      const Arr& b = r.arrs[j];
      if (a.bytes && b.bytes)
        CHECK(a.p + a.bytes <= b.p || b.p + b.bytes <= a.p, "%s/%s: %s overlaps %s", form, s.label, a.name.c_str(),
              b.name.c_str());
    }
  }
  for (size_t i = 0; i < need; ++i) buf[i] = (char)i;  // the whole measured size is the program's to write
  free(buf);
}

void check_chunk_rule() {
  const size_t big = (size_t)24 << 30;
  const int five = 5, zero = 0, minus = -3, huge = 1 << 30;
  CHECK(ksim_sweep_chunk(12, big, 1000, &five) == 5, "S = 12 under a cap of 5");
  CHECK(ksim_sweep_chunk(12, big, 1000, nullptr) == 12, "S = 12 without a cap");
  CHECK(ksim_sweep_chunk(12, big, 1000, &huge) == 12, "a cap above the chunk leaves it");
  CHECK(ksim_sweep_chunk(12, 999, 1000, nullptr) == 1, "budget / per == 0 still sweeps one scenario");
  CHECK(ksim_sweep_chunk(12, 0, 1000, nullptr) == 1, "no budget still sweeps one scenario");
  CHECK(ksim_sweep_chunk(12, 7999, 1000, nullptr) == 7, "budget / per below S");
  CHECK(ksim_sweep_chunk(12, 13000, 1000, nullptr) == 12, "budget / per above S gives S");
  CHECK(ksim_sweep_chunk(12, big, 1000, &zero) == 1, "a cap of 0 gives 1");
  CHECK(ksim_sweep_chunk(12, big, 1000, &minus) == 1, "a negative cap gives 1");
  CHECK(ksim_sweep_chunk(12, 999, 1000, &five) == 1, "a cap never raises the chunk");
  std::vector<int32_t> seq{5};
  while (seq.back() > 1) seq.push_back(ksim_sweep_halve(seq.back()));
  CHECK((seq == std::vector<int32_t>{5, 3, 2, 1}), "halving from 5");
  CHECK(ksim_sweep_halve(1) == 1, "1 stays 1");
}

}  // namespace

int main() {
  //                 label            N    P   S   T  NS NP  aw wcap CL  K leaves levels  weights absent rq spr
  const Shape shapes[] = {
      {"full",          1100, 40, 5, 7, 2, 3, 35, 3, 90, 4, 1152, 700, true, true, true, true},
      {"odd",           131, 7, 3, 1, 1, 1, 5, 7, 1, 1, 131, 33, false, true, true, false},
      {"no-scalars",    1100, 40, 5, 7, 0, 3, 35, 3, 90, 4, 1152, 700, true, true, true, true},
      {"no-ports",      1100, 40, 5, 7, 2, 0, 35, 3, 90, 4, 1152, 700, true, true, true, true},
      {"prefix-only",   1100, 0, 5, 7, 2, 3, 35, 3, 90, 4, 1152, 700, false, true, true, true},   // count == 0
      {"empty-prefix",  1100, 40, 5, 0, 2, 3, 35, 3, 90, 4, 1152, 700, false, true, true, true},  // T == 0
      {"no-records",    1100, 40, 5, 7, 2, 3, 35, 0, 90, 4, 1152, 700, true, true, true, true},   // wcap == 0
      {"no-node-sets",  1100, 40, 5, 7, 2, 3, 35, 3, 90, 4, 1152, 700, true, false, true, true},
      {"bare",          1, 1, 1, 0, 0, 0, 1, 0, 0, 1, 1, 1, false, false, false, false},
      {"spread-no-pairs", 64, 3, 2, 0, 0, 0, 2, 0, 0, 1, 64, 9, false, false, false, true},       // cnt_len == 0
  };
  for (const Shape& s : shapes)
    for (size_t C : {(size_t)1, (size_t)2, s.S}) {
      check_layout("general", general, s, C);
      if (s.P) {  // the resource-only forms take a pod range
        check_layout("scan", scan, s, C);
        check_layout("tree", tree, s, C);
      }
    }
  check_chunk_rule();
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
