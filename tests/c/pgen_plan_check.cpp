// pgen_plan_check.cpp — the launch geometry of the general persistent kernels (csrc/ksim_pgen_plan.h)
// under the system compiler, without a device: a stand-alone program with its own main
// (tests/test_pgen_plan_host.py compiles and runs it, once more under the address and
// undefined-behaviour sanitizers).  Every node count from 1 to 49,153 under every workgroup cap, with
// the single form forced and not, against byte models on either side of the LDS budget: an accepted
// plan must satisfy what ksim_launch_pgen / ksim_launch_pgen2 check before they launch, written out
// here a second time; a refusal must be a table no form holds.  Prints "ok" or the failed checks.
#include <cstdio>

#include "ksim_pgen_plan.h"

namespace {

int failures = 0;

#define CHECK(cond)                                                                                       \
  do {                                                                                                    \
    if (!(cond)) {                                                                                        \
      if (failures < 20)                                                                                  \
        std::printf("line %d: %s  (n %lld cap %d dual-allowed %d model %d hint %lld)\n", __LINE__, #cond, \
                    (long long)cur_n, cur_cap, (int)cur_allow, cur_model, (long long)cur_hint);           \
      ++failures;                                                                                         \
    }                                                                                                     \
  } while (0)

int64_t cur_n, cur_hint;
int cur_cap, cur_model;
bool cur_allow;

// A workgroup's LDS bytes, shaped like ksim_pgen_plan's: per-row columns, the static words, the dual
// form's second evaluation per row and its two more pod records, the dense deltas.
struct Model {
  size_t per_row, rec, dense;
  int32_t n_st;
  size_t budget;
  size_t operator()(int64_t chunk, bool dual, int32_t n_st_, int32_t hdense) const {
    return (size_t)chunk * (per_row + 2 * (size_t)n_st_ + (dual ? 40 : 0)) + rec * (dual ? 4 : 2) + (hdense ? dense : 0);
  }
};

constexpr size_t BUDGET = 154 * 1024;
const Model MODELS[] = {
    {73, 512, 0, 0, BUDGET},         // resource rows alone: everything fits, up to 1,024 rows
    {73, 1024, 4096, 40, BUDGET},    // static words and dense deltas that miss at the larger chunks
    {180, 2048, 8192, 3, BUDGET},    // 768 dual rows do not fit, 768 single rows do; 1,024 single rows do not
    {400, 6144, 16384, 16, BUDGET},  // a few hundred rows at the most
    {150, 512, 0, 0, 768 * 190 + 2048},      // the budget exactly at 768 dual rows ...
    {150, 512, 0, 0, 768 * 190 + 2048 - 1},  // ... and one byte short
    {100, 512, 0, 0, 1024 * 100 + 1024 - 1}, // one byte short of 1,024 single rows
};
constexpr int N_MODELS = sizeof MODELS / sizeof MODELS[0];

int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

void one(int64_t n, int cap, bool allow_dual, int mi, int64_t hint) {
  cur_n = n; cur_cap = cap; cur_allow = allow_dual; cur_model = mi; cur_hint = hint;
  const Model& m = MODELS[mi];
  KsimPgenPlanIn in{};
  in.n = n;
  in.max_grid = cap;
  in.allow_dual = allow_dual;
  in.hdense_ok = m.dense != 0;
  in.n_st = m.n_st;
  in.chunk_hint = hint;
  in.budget = m.budget;
  KsimPgenPlanOut o{};
  const bool ok = ksim_pgen_plan_geometry(in, m, &o);
  const int64_t gcap = (cap > 0 && cap < 256) ? cap : 256;
  const int64_t cmin1 = cdiv(n, gcap);                               // single form: the cap alone
  const int64_t cmin2 = cmin1 > cdiv(n, 64) ? cmin1 : cdiv(n, 64);   // dual form: and 64 workgroups
  const bool single_holds = cmin1 <= 4 * 256 && m(cmin1, false, 0, 0) <= m.budget;
  const bool dual_holds = allow_dual && cmin2 <= 4 * 192 && m(cmin2, true, 0, 0) <= m.budget;
  if (!ok) {
    CHECK(!single_holds && !dual_holds);  // a refusal: no form holds the table even at its smallest chunk
    return;
  }
  CHECK(single_holds || dual_holds);
  CHECK(o.dual == dual_holds);  // the dual form whenever it can launch the table
  // the launchers' conditions
  CHECK(o.grid >= 1 && o.grid <= 256 && o.grid <= gcap);
  CHECK((int64_t)o.grid * o.chunk >= n);
  CHECK((int64_t)(o.grid - 1) * o.chunk < n);  // no workgroup without rows
  CHECK(o.npt == 1 || o.npt == 2 || o.npt == 4);
  const int64_t rt = o.dual ? 192 : 256;
  CHECK(o.chunk >= 1 && o.chunk <= o.npt * rt);
  CHECK(o.npt == 1 || o.chunk > (o.npt / 2) * rt);  // the smallest instantiation that covers the chunk
  if (o.dual) CHECK(o.grid <= 64);
  // what was staged fits, is reported as planned, and was dropped only when it had to be
  CHECK(o.lds == m(o.chunk, o.dual, o.n_st, o.hdense) && o.lds <= m.budget);
  CHECK(o.n_st == 0 || o.n_st == m.n_st);
  CHECK(o.hdense == 0 || (o.hdense == 1 && o.dual && in.hdense_ok));
  const int32_t hd = (o.dual && in.hdense_ok) ? 1 : 0;
  if (o.n_st != m.n_st) CHECK(m(o.chunk, o.dual, m.n_st, hd) > m.budget);
  if (o.hdense != hd) CHECK(o.n_st == 0 && m(o.chunk, o.dual, 0, 1) > m.budget);
  // without a hint the search starts at one thread slot (or cmin) and only goes down
  const int64_t cmin = o.dual ? cmin2 : cmin1;
  CHECK(o.chunk >= cmin);
  if (!hint) CHECK(o.chunk <= (cmin > rt ? cmin : rt));
  else CHECK(o.chunk <= (hint > cmin ? hint : cmin));
}

void sweep() {
  const int caps[] = {0, 1, 2, 27, 40, 64, 65, 256};
  for (int64_t n = 1; n <= 49153; ++n)
    for (int cap : caps)
      for (int allow = 0; allow < 2; ++allow)  // 0: the lender / KSIM_PGEN_V1
        for (int mi = 0; mi < N_MODELS; ++mi) one(n, cap, allow != 0, mi, 0);
  // KSIM_PGEN_CHUNK: below cmin, at and around the thread-slot multiples, beyond four rows per thread
  const int64_t hints[] = {1, 3, 10, 191, 192, 193, 255, 256, 257, 384, 385, 512, 513, 768, 769, 1024, 1025, 5000};
  const int64_t ns[] = {1, 2, 64, 65, 191, 192, 193, 384, 385, 768, 769, 1000, 1024, 1025, 4097, 5000, 12288, 12289, 49152, 49153};
  for (int64_t n : ns)
    for (int64_t h : hints)
      for (int cap : caps)
        for (int allow = 0; allow < 2; ++allow)
          for (int mi = 0; mi < N_MODELS; ++mi) one(n, cap, allow != 0, mi, h);
}

// A capped handle whose rows exceed the dual form's 768 per workgroup runs the single form (up to
// 1,024), not a dual plan the launcher refuses; the dual form's own edges.
void named_cases() {
  cur_n = cur_hint = cur_cap = cur_model = 0;
  const Model& m = MODELS[0];
  KsimPgenPlanIn in{};
  in.allow_dual = true;
  in.budget = m.budget;
  KsimPgenPlanOut o{};
  auto plan = [&](int64_t n, int cap, int64_t hint = 0) {
    in.n = n; in.max_grid = cap; in.chunk_hint = hint;
    o = KsimPgenPlanOut{};
    return ksim_pgen_plan_geometry(in, m, &o);
  };
  CHECK(plan(768, 1) && o.dual && o.grid == 1 && o.chunk == 768 && o.npt == 4);
  CHECK(plan(769, 1) && !o.dual && o.grid == 1 && o.chunk == 769 && o.npt == 4);
  CHECK(plan(1024, 1) && !o.dual && o.grid == 1 && o.chunk == 1024 && o.npt == 4);
  CHECK(!plan(1025, 1));
  CHECK(plan(30720, 40) && o.dual && o.grid == 40 && o.chunk == 768);
  CHECK(plan(30721, 40) && !o.dual && o.grid == 40 && o.chunk == 769);
  CHECK(plan(40960, 40) && !o.dual && o.chunk == 1024);
  CHECK(!plan(40961, 40));
  CHECK(plan(49152, 0) && o.dual && o.grid == 64 && o.chunk == 768);
  CHECK(plan(49153, 0) && !o.dual && o.grid == 193 && o.chunk == 256);
  CHECK(plan(1, 1) && o.dual && o.grid == 1 && o.chunk == 1 && o.npt == 1);
  CHECK(plan(192, 1) && o.dual && o.npt == 1);
  CHECK(plan(193, 1) && o.dual && o.npt == 2 && o.chunk == 193);
  CHECK(plan(384, 1) && o.npt == 2);
  CHECK(plan(385, 1) && o.dual && o.npt == 4);
  CHECK(plan(193, 0) && o.dual && o.grid == 2 && o.chunk == 192);  // a last workgroup of one row
  // a hint never takes the dual form past 64 workgroups: the chunk is held at ceil(n / 64)
  CHECK(plan(4160, 0, 1) && o.dual && o.grid == 64 && o.chunk == 65);
  CHECK(plan(4161, 0, 1) && o.dual && o.grid == 64 && o.chunk == 66);
  in.allow_dual = false;
  CHECK(plan(4160, 0, 1) && !o.dual && o.grid == 245 && o.chunk == 17);
  CHECK(plan(256, 1) && o.npt == 1);
  CHECK(plan(257, 1) && o.npt == 2);
  CHECK(plan(512, 1) && o.npt == 2);
  CHECK(plan(513, 1) && o.npt == 4);
  CHECK(!plan(0, 0) && !plan(-1, 0));
}

}  // namespace

int main() {
  sweep();
  named_cases();
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
