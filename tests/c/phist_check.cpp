// Host check of csrc/ksim_phist.h, the bookkeeping of the fast kernel's histogram sub-form: build
// from a cache column, one row's move, and (F, M, C) with two adjusted buckets, each against a
// recount of the column.  Stand-alone (own main), compiled by tests/test_phist_host.py with the
// system compiler; prints "ok" and exits 0, or says what differed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ksim_phist.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

int fails = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      if (fails++ < 20) {                     \
        std::printf("%s:%d: ", __FILE__, __LINE__); \
        std::printf(__VA_ARGS__);             \
        std::printf("\n");                    \
      }                                       \
    }                                         \
  } while (0)

struct Stats {
  int32_t f, m, c;
};

// the recount: what the row scan of the plain cached form computes
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

struct Hist {
  uint16_t row[KSIM_PHIST_BUCKETS];
  void build(const std::vector<int16_t>& col) {
    uint32_t words[KSIM_PHIST_BUCKETS / 2];
    khist::build(words, col.data(), (int)col.size());
    static_assert(sizeof(words) == sizeof(row), "two counts a word");
    std::memcpy(row, words, sizeof(row));  // the kernel reads the words as uint16[64] (little-endian)
  }
  void check(const std::vector<int16_t>& col, const char* what) const {
    int32_t cnt[KSIM_PHIST_BUCKETS] = {};
    for (int16_t e : col)
      if (e >= 0) cnt[e] += 1;
    for (int s = 0; s < KSIM_PHIST_BUCKETS; ++s) CHECK(row[s] == cnt[s], "%s: bucket %d holds %d, recount %d", what, s, row[s], cnt[s]);
    Stats got;
    khist::stats(row, -1, -1, &got.f, &got.m, &got.c);
    const Stats want = recount(col);
    CHECK(got.f == want.f && got.m == want.m && got.c == want.c, "%s: stats (%d, %d, %d), recount (%d, %d, %d)", what, got.f,
          got.m, got.c, want.f, want.m, want.c);
  }
};

// One commit as the owner does it: the corrected statistics from the untouched row first (what
// the fix granule carries), then the move, then a recount of everything.
void commit(Hist& h, std::vector<int16_t>& col, int j, int e_new, const char* what) {
  const int e_old = col[j];
  Stats got;
  khist::stats(h.row, e_old, e_new, &got.f, &got.m, &got.c);
  col[j] = (int16_t)e_new;
  const Stats want = recount(col);
  CHECK(got.f == want.f && got.m == want.m && got.c == want.c,
        "%s: row %d %d -> %d: adjusted stats (%d, %d, %d), recount (%d, %d, %d)", what, j, e_old, e_new, got.f, got.m, got.c,
        want.f, want.m, want.c);
  khist::move(h.row, e_old, e_new);
  h.check(col, what);
}

void directed() {
  CHECK(khist::top(0) == -1, "top of an empty row");
  for (int s = 0; s < KSIM_PHIST_BUCKETS; ++s) {
    CHECK(khist::top(1ull << s) == s && khist::top((1ull << s) | 1ull) == s, "top of bucket %d", s);
    CHECK(khist::word(s) == s / 2 && khist::unit(s) == (s % 2 ? 65536u : 1u), "word / unit of bucket %d", s);
  }
  Hist h;
  // a bucket emptied to the next one: the only row at the top drops below the second bucket
  std::vector<int16_t> col = {20, 17, 17, 3, -1, 0};
  h.build(col);
  h.check(col, "built");
  commit(h, col, 0, 5, "top bucket emptied to the next");
  CHECK(recount(col).m == 17 && recount(col).c == 2, "the next bucket took over");
  // ... and to a gap of empty buckets, down to bucket 0
  commit(h, col, 1, -1, "a row turning unfit at the top");
  commit(h, col, 2, -1, "the top bucket emptied across a gap");
  CHECK(recount(col).m == 5, "bucket 5 after the gap");
  // a row entering above the top, from a bucket and from unfit
  commit(h, col, 3, 40, "a row entering above the top");
  commit(h, col, 4, 41, "an unfit row entering above the top");
  // score 63, the last lane
  commit(h, col, 5, 63, "score 63");
  commit(h, col, 0, 63, "a second row at 63");
  commit(h, col, 5, 62, "63 -> 62");
  commit(h, col, 0, -1, "63 emptied");
  // a row that stays where it is
  commit(h, col, 3, 40, "no move");
  commit(h, col, 1, -1, "unfit stays unfit");
  // every row unfit, one by one: F = 1, then F = 0
  for (int j = 0; j < (int)col.size(); ++j) commit(h, col, j, -1, "draining");
  CHECK(recount(col).f == 0, "drained");
  commit(h, col, 2, 0, "the first fit row, at score 0");
  // a full workgroup at one score: 1,568 rows in bucket 63 and in bucket 62, the neighbours of a word
  col.assign(1568, 63);
  h.build(col);
  h.check(col, "1568 rows at 63");
  col.assign(1568, 62);
  col[7] = 63;
  h.build(col);
  h.check(col, "1567 rows at 62, one at 63");
  commit(h, col, 7, 62, "1568 rows at 62");
}

void random_runs() {
  for (int run = 0; run < 400; ++run) {
    const int n = 1 + (int)(rnd() % 300);
    // few distinct scores (ties everywhere), a band, or the whole range; some rows unfit
    const int span = run % 3 == 0 ? 2 : run % 3 == 1 ? 12 : KSIM_PHIST_BUCKETS;
    const int base = (int)(rnd() % (KSIM_PHIST_BUCKETS - span + 1));
    const int unfit = (int)(rnd() % 4);  // out of 4
    auto draw = [&]() -> int { return (int)(rnd() % 4) < unfit ? -1 : base + (int)(rnd() % span); };
    std::vector<int16_t> col(n);
    for (auto& e : col) e = (int16_t)draw();
    Hist h;
    h.build(col);
    h.check(col, "random build");
    for (int step = 0; step < 200; ++step) {
      const int j = (int)(rnd() % n);
      // mostly what a commit does — the score drifts or the row turns unfit — and any move at all
      int e = draw();
      if (step % 2 && col[j] >= 0) e = rnd() % 3 ? (col[j] > 0 ? col[j] - 1 : 0) : -1;
      commit(h, col, j, e, "random commit");
    }
    // the build from the column as it now stands equals the moved histogram
    Hist again;
    again.build(col);
    CHECK(std::memcmp(again.row, h.row, sizeof(h.row)) == 0, "rebuild after the commits");
  }
}

}  // namespace

int main() {
  directed();
  random_runs();
  if (fails) {
    std::printf("%d checks failed\n", fails);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
