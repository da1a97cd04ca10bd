// sddmm_schedule_check.cpp — sddmm_schedule() and sddmm_first_bad_row() of csrc/slq_sddmm.hpp over seeded random patterns (row
// lengths around the long-row threshold, empty rows, full rows, sizes around the 64-row block), with what the kernel relies on
// checked on every answer: every stored nonzero owned by exactly one item, a short item inside one aligned block of 64 rows with
// no long row in it, a long item a single long row. Then damaged patterns: the validation names the row. A stand-alone host
// program for the sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I primate_amd/csrc scripts/sddmm_schedule_check.cpp -o sddmm_schedule_check
//   ./sddmm_schedule_check
// It includes nothing but the header under test; no device, no library.
#include "slq_sddmm.hpp"

#include <cstdio>
#include <random>
#include <vector>

using namespace slq;

static long g_cases = 0, g_failed = 0;
#define CHECK(cond)                                                                 \
  do {                                                                              \
    if (!(cond)) {                                                                  \
      if (g_failed++ < 20) fprintf(stderr, "case %ld: %s failed\n", g_cases, #cond); \
    }                                                                               \
  } while (0)

static void check(int64_t n, const std::vector<int32_t> &rp, const std::vector<int32_t> &ci) {
  ++g_cases;
  const int64_t nnz = rp[(size_t)n];
  CHECK(sddmm_first_bad_row(n, nnz, rp.data(), ci.data()) == -1);
  const SddmmSchedule S = sddmm_schedule(n, rp.data());
  std::vector<int> owners((size_t)nnz, 0);
  int64_t nlong = 0;
  for (const SddmmItem &it : S.items) {
    int64_t e0, e1;
    sddmm_item_range(it, rp.data(), &e0, &e1);
    CHECK(it.row0 >= 0 && it.row0 < n && e0 < e1 && e1 <= nnz);
    if (it.nrows == 0) {
      ++nlong;
      CHECK(rp[(size_t)it.row0 + 1] - rp[(size_t)it.row0] > kSddmmLongRow);
    } else {
      CHECK(it.nrows <= 64 && it.row0 + it.nrows <= n && it.row0 / 64 == (it.row0 + it.nrows - 1) / 64);
      for (int64_t r = it.row0; r < it.row0 + it.nrows; ++r) CHECK(rp[(size_t)r + 1] - rp[(size_t)r] <= kSddmmLongRow);
    }
    for (int64_t e = e0; e < e1; ++e) ++owners[(size_t)e];
  }
  for (int64_t e = 0; e < nnz; ++e) CHECK(owners[(size_t)e] == 1);
  CHECK(nlong == S.nlong && S.grid == ((int64_t)S.items.size() + kSddmmWaves - 1) / kSddmmWaves);
  if (nnz == 0) CHECK(S.items.empty() && S.grid == 0);
}

int main() {
  std::mt19937_64 rng(12345);
  for (int64_t n : {1, 2, 63, 64, 65, 127, 128, 143, 300, 1000}) {
    for (int style = 0; style < 6; ++style) {
      std::vector<int32_t> rp((size_t)n + 1, 0), ci;
      for (int64_t r = 0; r < n; ++r) {
        int64_t len = 0;
        switch (style) {
          case 0: len = 0; break;                                                   // nnz = 0
          case 1: len = (int64_t)(rng() % 8); break;                                // short rows, some empty
          case 2: len = kSddmmLongRow - 1 + (int64_t)(rng() % 3); break;            // around the threshold
          case 3: len = (rng() % 16 == 0) ? n : (int64_t)(rng() % 4); break;        // a few full rows
          case 4: len = (r % 64 == 0 || r % 64 == 63) ? kSddmmLongRow + 5 : 3; break;  // long rows at the block edges
          default: len = n; break;                                                  // dense
        }
        len = std::min(len, n);
        for (int64_t q = 0; q < len; ++q) ci.push_back((int32_t)(rng() % (uint64_t)n));  // (unsorted, duplicates: the pattern is taken as given)
        rp[(size_t)r + 1] = (int32_t)ci.size();
      }
      check(n, rp, ci);
      // damaged copies: the first offending row is named
      const int64_t nnz = rp[(size_t)n];
      if (nnz > 0) {
        ++g_cases;
        int64_t row = 0;
        while (rp[(size_t)row + 1] == rp[(size_t)row]) ++row;  // first non-empty row
        std::vector<int32_t> bad = ci;
        bad[(size_t)rp[(size_t)row]] = (int32_t)n;
        CHECK(sddmm_first_bad_row(n, nnz, rp.data(), bad.data()) == row);
        bad[(size_t)rp[(size_t)row]] = -1;
        CHECK(sddmm_first_bad_row(n, nnz, rp.data(), bad.data()) == row);
        std::vector<int32_t> rq = rp;
        rq[(size_t)n] += 1;  // past the arrays: refused before colind is read there
        CHECK(sddmm_first_bad_row(n, nnz, rq.data(), ci.data()) == n - 1);
        rq = rp;
        rq[0] = 1;
        CHECK(sddmm_first_bad_row(n, nnz, rq.data(), ci.data()) == 0);
        if (n >= 2 && rp[(size_t)row + 1] > 0) {
          rq = rp;
          rq[(size_t)row + 1] = -1;  // goes down at `row`
          CHECK(sddmm_first_bad_row(n, nnz, rq.data(), ci.data()) == row);
        }
      }
    }
  }
  printf("sddmm_schedule_check: %ld cases, %ld failed checks\n", g_cases, g_failed);
  return g_failed ? 1 : 0;
}
