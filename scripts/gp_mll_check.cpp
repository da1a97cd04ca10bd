// gp_mll_check.cpp — H of csrc/slq_kernelprecond.hpp's precond_finish: with the Gram matrix A = L^T L = V diag(t) V^T of
// precond_jacobi, H = V diag(1 / (t + sigma2)) V^T is the inverse of A + sigma2 I: max |H (A + sigma2 I) - I| <= 64 eps r cond,
// cond = (t_max + sigma2) / sigma2; H is exactly symmetric, finite, and zero in the rows and columns of the padding (rpad > r); G of
// the same call is what it is without H (the default argument). The matrix families are those of scripts/kernelprecond_check.cpp:
// seeded Gram matrices up to r = 256 - full rank, rank-deficient, eigenvalues over 16 decades, zero columns - at three noise levels.
// A stand-alone host program for the sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I primate_amd/csrc scripts/gp_mll_check.cpp -o gp_mll_check
//   ./gp_mll_check
// It includes nothing but the header under test; no device, no library.
#include "slq_kernelprecond.hpp"

#include <cstdio>
#include <random>
#include <vector>

using namespace slq;

static long g_cases = 0, g_failed = 0;
static double g_worst = 0.0;  // the largest error over its bound
#define CHECK(cond)                                                                 \
  do {                                                                              \
    if (!(cond)) {                                                                  \
      if (g_failed++ < 20) fprintf(stderr, "case %ld: %s failed\n", g_cases, #cond); \
    }                                                                               \
  } while (0)

// A = X^T X for a seeded m x r matrix X whose column c is scaled by scale[c] (0: a zero column)
static std::vector<double> gram_matrix(int r, int m, const std::vector<double> &scale, unsigned seed) {
  std::mt19937_64 rng(seed);
  std::normal_distribution<double> N(0.0, 1.0);
  std::vector<double> X((size_t)m * r), A((size_t)r * r, 0.0);
  for (int i = 0; i < m; ++i)
    for (int c = 0; c < r; ++c) X[(size_t)i * r + c] = N(rng) * scale[(size_t)c];
  for (int a = 0; a < r; ++a)
    for (int b = a; b < r; ++b) {
      double s = 0.0;
      for (int i = 0; i < m; ++i) s += X[(size_t)i * r + a] * X[(size_t)i * r + b];
      A[(size_t)a * r + b] = A[(size_t)b * r + a] = s;
    }
  return A;
}

static void check_h(int r, int m, const std::vector<double> &scale, unsigned seed, double sigma2) {
  ++g_cases;
  const std::vector<double> A0 = gram_matrix(r, m, scale, seed);
  std::vector<double> A = A0, V((size_t)r * r), t((size_t)r);
  CHECK(precond_jacobi(r, A.data(), V.data(), t.data()) < kPrecondJacobiSweeps);
  const int rpad = precond_rpad(r);
  std::vector<double> G((size_t)rpad * rpad, -1.0), G0((size_t)rpad * rpad, -2.0), H((size_t)rpad * rpad, -3.0);
  const PrecondSpectrum sp = precond_finish(1000, r, rpad, V.data(), t.data(), sigma2, G.data(), H.data());
  const PrecondSpectrum sp0 = precond_finish(1000, r, rpad, V.data(), t.data(), sigma2, G0.data());
  CHECK(sp.logdet_p == sp0.logdet_p && sp.t_max == sp0.t_max && G == G0);  // H changes nothing else
  for (int i = 0; i < rpad; ++i)
    for (int j = 0; j < rpad; ++j) {
      const double h = H[(size_t)i * rpad + j];
      CHECK(std::isfinite(h) && h == H[(size_t)j * rpad + i]);
      if (i >= r || j >= r) CHECK(h == 0.0);
    }
  const double eps = std::numeric_limits<double>::epsilon();
  const double cond = (sp.t_max + sigma2) / sigma2, bound = 64.0 * eps * r * cond;
  double worst = 0.0;
  for (int i = 0; i < r; ++i)
    for (int j = 0; j < r; ++j) {
      double s = 0.0;
      for (int k = 0; k < r; ++k) s += H[(size_t)i * rpad + k] * (A0[(size_t)k * r + j] + (k == j ? sigma2 : 0.0));
      worst = std::max(worst, std::fabs(s - (i == j ? 1.0 : 0.0)));
    }
  CHECK(worst <= bound);
  g_worst = std::max(g_worst, worst / bound);
  CHECK(precond_h(-1e-9, sigma2) == 1.0 / sigma2 && precond_h(0.0, sigma2) == 1.0 / sigma2);  // (a rounded zero eigenvalue counts as 0)
}

int main() {
  for (double sigma2 : {1e-6, 1e-4, 1e-2})
    for (int r : {1, 2, 5, 16, 33, 64, 128, 256}) {
      std::vector<double> ones((size_t)r, 1.0), decay((size_t)r), holes((size_t)r);
      for (int c = 0; c < r; ++c) decay[(size_t)c] = std::pow(10.0, -8.0 * c / std::max(r - 1, 1)), holes[(size_t)c] = c % 3 == 2 ? 0.0 : 1.0 / (1 + c);
      check_h(r, 2 * r + 3, ones, 1u + r, sigma2);   // full rank
      check_h(r, r / 2 + 1, ones, 2u + r, sigma2);   // rank-deficient
      check_h(r, 2 * r + 3, decay, 3u + r, sigma2);  // eigenvalues over 16 decades
      check_h(r, 2 * r + 3, holes, 4u + r, sigma2);  // zero columns: the Gram matrix of a factor that stopped early
    }
  printf("gp_mll_check: %ld cases, %ld failed checks, worst |H (A + sigma2 I) - I| / (64 eps r cond) = %.3g\n", g_cases, g_failed, g_worst);
  return g_failed ? 1 : 0;
}
