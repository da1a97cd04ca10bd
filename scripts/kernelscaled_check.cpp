// kernelscaled_check.cpp — the host part of the diagonally scaled kernel operator (csrc/slq_kernelop.hpp):
// kernel_validate_diag_scale() over good and damaged scales in both dtypes - the first bad entry is named, with its value; the length
// is checked before any entry is read (a short array is never indexed past its end: the arrays here are allocated to their exact
// length, which is what the address sanitizer watches); zeros, denormals and the largest finite number of the dtype are accepted;
// what is finite in double and not in float is refused for float only - and kernel_bad_message() on every answer. A stand-alone host
// program for the sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I primate_amd/csrc scripts/kernelscaled_check.cpp -o kernelscaled_check
//   ./kernelscaled_check
// It includes nothing but the header under test; no device, no library.
#include "slq_kernelop.hpp"

#include <cstring>
#include <limits>
#include <memory>
#include <random>
#include <string>

using namespace slq;

static long g_cases = 0, g_failed = 0;
#define CHECK(cond)                                                                 \
  do {                                                                              \
    if (!(cond)) {                                                                  \
      if (g_failed++ < 20) fprintf(stderr, "case %ld: %s failed\n", g_cases, #cond); \
    }                                                                               \
  } while (0)

static char g_msg[256];
static int what(const KernelBad &b) {
  ++g_cases;
  kernel_bad_message(b, g_msg, sizeof g_msg);
  CHECK(strlen(g_msg) > 10 && strlen(g_msg) < sizeof g_msg - 1);
  return b.what;
}

// an array of exactly n doubles on the heap: one entry past its end is the sanitizer's
static std::unique_ptr<double[]> scale(int64_t n, std::mt19937_64 &rng) {
  std::unique_ptr<double[]> c(new double[(size_t)n]);
  std::uniform_real_distribution<double> U(std::log(0.1), std::log(10.0));
  for (int64_t i = 0; i < n; ++i) c[(size_t)i] = std::exp(U(rng));
  return c;
}

int main() {
  std::mt19937_64 rng(11);
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  for (int64_t n : {1, 2, 15, 16, 17, 257, 1000, 65536}) {
    auto c = scale(n, rng);
    CHECK(what(kernel_validate_diag_scale<double>(n, c.get(), n)) == KERNEL_OK);
    CHECK(what(kernel_validate_diag_scale<float>(n, c.get(), n)) == KERNEL_OK);
    // the length comes first, and a wrong one reads no entry (nc < n would otherwise run past the end of a short array)
    for (int64_t nc : {(int64_t)0, n - 1, n + 1, (int64_t)-1}) {
      if (nc == n) continue;
      auto shorter = scale(std::max<int64_t>(nc, 1), rng);
      const KernelBad b = kernel_validate_diag_scale<double>(n, shorter.get(), nc);
      CHECK(what(b) == KERNEL_BAD_SCALE_LENGTH && b.row == nc && b.col == n);
      CHECK(strstr(g_msg, (std::to_string(nc) + " entries").c_str()) != nullptr);
    }
    // zeros (a saturated likelihood), denormals and the largest finite number are fine
    c[0] = 0.0;
    c[(size_t)(n - 1)] = 0.0;
    CHECK(what(kernel_validate_diag_scale<double>(n, c.get(), n)) == KERNEL_OK);
    c[(size_t)(n / 2)] = std::numeric_limits<double>::denorm_min();
    CHECK(what(kernel_validate_diag_scale<float>(n, c.get(), n)) == KERNEL_OK);  // (rounds to 0 in float: allowed)
    c[(size_t)(n / 2)] = std::numeric_limits<double>::max();
    CHECK(what(kernel_validate_diag_scale<double>(n, c.get(), n)) == KERNEL_OK);
    {
      const KernelBad b = kernel_validate_diag_scale<float>(n, c.get(), n);  // finite in double, not in float
      CHECK(what(b) == KERNEL_BAD_SCALE && b.row == n / 2);
    }
    c[(size_t)(n / 2)] = (double)std::numeric_limits<float>::max();
    CHECK(what(kernel_validate_diag_scale<float>(n, c.get(), n)) == KERNEL_OK);
    c[(size_t)(n / 2)] = -0.0;  // (-0 >= 0: accepted, and it is a zero)
    CHECK(what(kernel_validate_diag_scale<double>(n, c.get(), n)) == KERNEL_OK);
    // the FIRST bad entry is named, with its value, at every position including the two ends
    for (double badv : {-1.0, -1e-300, nan, inf, -inf}) {
      for (int64_t at : {(int64_t)0, n / 3, n - 1}) {
        auto d = scale(n, rng);
        d[(size_t)at] = badv;
        if (at + 1 < n) d[(size_t)(n - 1)] = nan;  // (a later one is not what is reported)
        const KernelBad b = kernel_validate_diag_scale<double>(n, d.get(), n);
        CHECK(what(b) == KERNEL_BAD_SCALE && b.row == at && (std::isnan(badv) ? std::isnan(b.value) : b.value == badv));
        CHECK(strstr(g_msg, ("diag_scale[" + std::to_string(at) + "]").c_str()) != nullptr);
        const KernelBad bf = kernel_validate_diag_scale<float>(n, d.get(), n);
        CHECK(what(bf) == KERNEL_BAD_SCALE && bf.row == at);
      }
    }
  }
  // the other validators are untouched by the new codes: a good parameter set is still KERNEL_OK, and the message table has no hole
  const double ls1[1] = {0.5};
  CHECK(what(kernel_validate_parameters(3, ls1, 1, 1.0, 0.0)) == KERNEL_OK);
  for (int w = KERNEL_OK; w <= KERNEL_BAD_SCALE; ++w) {
    KernelBad b;
    b.what = w, b.row = 3, b.col = 4, b.value = 0.5;
    what(b);
    CHECK(w == KERNEL_OK || strstr(g_msg, ": ok") == nullptr);
  }
  printf("kernelscaled_check: %ld cases, %ld failed checks\n", g_cases, g_failed);
  return g_failed ? 1 : 0;
}
