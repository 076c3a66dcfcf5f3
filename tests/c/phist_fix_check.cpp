// Host check of khist::fix (csrc/ksim_phist.h): the owner's fix of the fast kernel's histogram
// sub-form as a function of the class's top two buckets, (F0, M1, C1, M2, C2, e_old, e_new) ->
// (F', M', C'), against khist::stats on the row and against a recount of the column.  Every case
// of the arithmetic is counted (KSIM_PHIST_TAKEN) and none may stay at zero.  Stand-alone (own
// main), compiled by tests/test_phist_fix_host.py with the system compiler; prints "ok" and exits
// 0, or says what differed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {
constexpr int NCASE = 10;
long taken[NCASE];
const char* const case_name[NCASE] = {
    "the row leaves the top bucket", "the row leaves another bucket or none", "the top bucket keeps rows",
    "the second bucket becomes the top", "nothing is left", "the row turns or stays unfit", "the row enters an empty class",
    "the row enters above the top", "the row enters the top bucket", "the row enters below the top"};
}  // namespace
#define KSIM_PHIST_TAKEN(k) (taken[(k)] += 1)

#include "ksim_phist.h"

namespace {

uint64_t rng_state = 0x243F6A8885A308D3ull;
uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

int fails = 0;
#define CHECK(cond, ...)                            \
  do {                                              \
    if (!(cond)) {                                  \
      if (fails++ < 20) {                           \
        std::printf("%s:%d: ", __FILE__, __LINE__); \
        std::printf(__VA_ARGS__);                   \
        std::printf("\n");                          \
      }                                             \
    }                                               \
  } while (0)

struct Stats {
  int32_t f, m, c;
  bool operator==(const Stats& o) const { return f == o.f && m == o.m && c == o.c; }
};

// what the row waves take from the class's histogram row: the sum and the top two buckets
struct Top2 {
  int32_t f;
  int m1;
  int32_t c1;
  int m2;
  int32_t c2;
};
Top2 top_two(const uint16_t* row) {
  uint64_t ne = 0;
  Top2 t{0, -1, 0, -1, 0};
  for (int s = 0; s < KSIM_PHIST_BUCKETS; ++s) {
    t.f += row[s];
    ne |= (uint64_t)(row[s] != 0) << s;
  }
  t.m1 = khist::top(ne);
  if (t.m1 >= 0) {
    t.c1 = row[t.m1];
    t.m2 = khist::top(ne & ~(1ull << t.m1));
    if (t.m2 >= 0) t.c2 = row[t.m2];
  }
  return t;
}

Stats fixed(const uint16_t* row, int e_old, int e_new) {
  const Top2 t = top_two(row);
  Stats s;
  int32_t m;
  khist::fix(t.f, t.m1, t.c1, t.m2, t.c2, e_old, e_new, &s.f, &m, &s.c);
  s.m = m;
  return s;
}

// the fix of a row whose histogram holds e_old (or e_old = -1) against khist::stats on the row
void against_stats(const uint16_t* row, int e_old, int e_new, const char* what) {
  Stats want;
  khist::stats(row, e_old, e_new, &want.f, &want.m, &want.c);
  const Stats got = fixed(row, e_old, e_new);
  CHECK(got == want, "%s: %d -> %d: fix (%d, %d, %d), stats (%d, %d, %d)", what, e_old, e_new, got.f, got.m, got.c, want.f,
        want.m, want.c);
  CHECK(got.c != 0 || got.m == -1, "%s: %d -> %d: M = %d with C = 0", what, e_old, e_new, got.m);
}

// Every (e_old, e_new) in {-1, 0..63}^2 over histograms with 0 to 3 non-empty buckets and top
// counts 1 and 2.  The moved row is one of the histogram's rows, so a histogram is tried with
// an e_old only where that bucket holds a row; e_old = -1 (an unfit row) goes with all of them.
void exhaustive() {
  const int places[][3] = {{-1, -1, -1}, {0, -1, -1}, {63, -1, -1}, {31, -1, -1}, {1, 0, -1},   {63, 62, -1},
                           {63, 0, -1},  {40, 7, -1}, {2, 1, 0},    {63, 62, 61}, {63, 30, 0}, {50, 49, 3}};
  for (const auto& pl : places)
    for (int c_top = 1; c_top <= 2; ++c_top)
      for (int c_rest = 1; c_rest <= 2; ++c_rest) {
        uint16_t row[KSIM_PHIST_BUCKETS] = {};
        for (int k = 0; k < 3; ++k)
          if (pl[k] >= 0) row[pl[k]] = (uint16_t)(k == 0 ? c_top : c_rest);
        for (int e_old = -1; e_old < KSIM_PHIST_BUCKETS; ++e_old) {
          if (e_old >= 0 && row[e_old] == 0) continue;
          for (int e_new = -1; e_new < KSIM_PHIST_BUCKETS; ++e_new) against_stats(row, e_old, e_new, "exhaustive");
        }
      }
  // the other buckets' rows, once the row that moves is added to any bucket of any of them: the
  // histogram then holds e_old by construction, for every e_old
  for (const auto& pl : places)
    for (int c_top = 1; c_top <= 2; ++c_top)
      for (int e_old = 0; e_old < KSIM_PHIST_BUCKETS; ++e_old) {
        uint16_t row[KSIM_PHIST_BUCKETS] = {};
        for (int k = 0; k < 3; ++k)
          if (pl[k] >= 0) row[pl[k]] = (uint16_t)(k == 0 ? c_top : 1);
        row[e_old] += 1;
        for (int e_new = -1; e_new < KSIM_PHIST_BUCKETS; ++e_new) against_stats(row, e_old, e_new, "exhaustive, row added");
      }
}

Stats recount(const std::vector<int16_t>& col) {
  Stats s{0, -1, 0};
  for (int16_t e : col) {
    if (e < 0) continue;
    s.f += 1;
    if (e > s.m) { s.m = e; s.c = 1; }
    else if (e == s.m) s.c += 1;
  }
  return s;
}

struct Column {
  std::vector<int16_t> col;
  uint16_t row[KSIM_PHIST_BUCKETS];
  explicit Column(std::vector<int16_t> c) : col(std::move(c)) {
    uint32_t words[KSIM_PHIST_BUCKETS / 2];
    khist::build(words, col.data(), (int)col.size());
    std::memcpy(row, words, sizeof(row));
  }
  // one commit as the kernel does it: the fix from the untouched row, then the move, then a recount
  void commit(int j, int e_new, const char* what) {
    const int e_old = col[j];
    against_stats(row, e_old, e_new, what);
    const Stats got = fixed(row, e_old, e_new);
    khist::move(row, e_old, e_new);
    col[j] = (int16_t)e_new;
    const Stats want = recount(col);
    CHECK(got == want, "%s: row %d %d -> %d: fix (%d, %d, %d), recount (%d, %d, %d)", what, j, e_old, e_new, got.f, got.m, got.c,
          want.f, want.m, want.c);
  }
};

void directed() {
  {  // F0 = 1 going to no fit row, and back
    Column c({-1, 9, -1});
    c.commit(1, -1, "the only fit row turns unfit");
    CHECK(recount(c.col).f == 0, "no fit row");
    c.commit(0, -1, "unfit stays unfit in an empty class");
    c.commit(2, 0, "the first fit row, at score 0");
  }
  {  // a top bucket of one row emptied across a gap
    Column c({40, 3, 3, -1});
    c.commit(0, 1, "the top bucket of one row emptied across a gap, the row landing below the next");
    CHECK(recount(c.col).m == 3 && recount(c.col).c == 2, "bucket 3 took over");
  }
  {  // e_new below, on, between and above the old top two
    const int16_t base[] = {30, 20, 20, 10, 10, 10};
    for (int e_new : {5, 10, 15, 20, 25, 30, 35, -1}) {
      Column c(std::vector<int16_t>(base, base + 6));
      c.commit(0, e_new, "the only top row moves: below, on, between, above the top two");
      Column d(std::vector<int16_t>(base, base + 6));
      d.commit(1, e_new, "a row of the second bucket moves");
      Column e(std::vector<int16_t>(base, base + 6));
      e.commit(3, e_new, "a row below the top two moves");
    }
  }
  {  // score 63
    Column c({62, 62, 0});
    c.commit(2, 63, "a row enters bucket 63");
    c.commit(0, 63, "a second row at 63");
    c.commit(2, 62, "63 -> 62");
    c.commit(0, -1, "63 emptied");
    c.commit(1, 63, "62 -> 63");
  }
}

void random_runs() {
  for (int run = 0; run < 300; ++run) {
    const int n = run < 4 ? 1568 : 1 + (int)(rnd() % 1568);
    const int span = run % 3 == 0 ? 2 : run % 3 == 1 ? 12 : KSIM_PHIST_BUCKETS;
    const int base = (int)(rnd() % (KSIM_PHIST_BUCKETS - span + 1));
    const int unfit = (int)(rnd() % 4);  // out of 4
    auto draw = [&]() -> int { return (int)(rnd() % 4) < unfit ? -1 : base + (int)(rnd() % span); };
    std::vector<int16_t> col(n);
    for (auto& e : col) e = (int16_t)draw();
    Column c(col);
    for (int step = 0; step < 200; ++step) {
      // a commit goes to a row at the top; its score drifts down or the row turns unfit — and any move at all
      int j = (int)(rnd() % n);
      const Stats s = recount(c.col);
      if (step % 2 && s.m >= 0)
        while (c.col[j] != s.m) j = (j + 1) % n;
      int e = draw();
      if (step % 4 == 1 && c.col[j] >= 0) e = rnd() % 3 ? (c.col[j] > 0 ? c.col[j] - 1 : 0) : -1;
      c.commit(j, e, "random commit");
    }
    Column again(c.col);
    CHECK(std::memcmp(again.row, c.row, sizeof(c.row)) == 0, "rebuild after the commits");
  }
}

}  // namespace

int main() {
  exhaustive();
  directed();
  random_runs();
  for (int k = 0; k < NCASE; ++k) CHECK(taken[k] > 0, "case never taken: %s", case_name[k]);
  if (fails) {
    std::printf("%d checks failed\n", fails);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
