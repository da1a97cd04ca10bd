// kernelprecond_check.cpp — the host part of csrc/slq_kernelprecond.hpp: the row slabs of the apply (precond_apply_slabs) are a
// partition of the rows into runs of whole 16-row tiles for n around multiples of 16, every column count 1 .. 260 and three chip
// sizes, and the scratch an apply is given holds them; cyclic Jacobi (precond_jacobi) on seeded positive semi-definite Gram
// matrices up to r = 256 - full rank, rank-deficient, with zero columns, with eigenvalues over 16 decades - reconstructs
// V diag(t) V^T to 64 eps r |A| with orthonormal V; g(t) (precond_g) is finite, positive and non-increasing from 0 through the
// denormals up to 1e12 sigma2, and precond_finish's G is symmetric with zero padding. A stand-alone host program for the sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I primate_amd/csrc scripts/kernelprecond_check.cpp -o kernelprecond_check
//   ./kernelprecond_check
// It includes nothing but the header under test; no device, no library.
#include "slq_kernelprecond.hpp"

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

static void check_slabs(int64_t n, int64_t cols, int cus) {
  ++g_cases;
  const PrecondSlabs S = precond_apply_slabs(n, cols, cus);
  CHECK(S.nslabs >= 1 && S.nslabs <= kPrecondMaxSlabs);
  CHECK(S.rows_per_slab >= 16 && S.rows_per_slab % 16 == 0);
  // slab z is the rows [z rows_per_slab, min(n, (z + 1) rows_per_slab)): what k_precond_lt computes from its block index
  int64_t covered = 0;
  for (int z = 0; z < S.nslabs; ++z) {
    const int64_t r0 = (int64_t)z * S.rows_per_slab, r1 = std::min<int64_t>(n, r0 + S.rows_per_slab);
    CHECK(r0 == covered && r0 < r1);  // contiguous, no empty slab
    covered = r1;
  }
  CHECK(covered == n);
  const int64_t bpad = precond_bpad(cols);
  CHECK(bpad >= cols && bpad % kPrecondColsPerWg == 0 && bpad - cols < kPrecondColsPerWg);
  for (int rpad : {16, 48, 256}) {
    CHECK(precond_scratch_words(n, cols, rpad, cus) == (size_t)(S.nslabs + 1) * (size_t)bpad * (size_t)rpad);
    CHECK(precond_scratch_words(n, cols, rpad, cus) <= precond_scratch_bound_words(cols, rpad));
  }
}

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

static void check_jacobi(int r, int m, const std::vector<double> &scale, unsigned seed) {
  ++g_cases;
  const std::vector<double> A0 = gram_matrix(r, m, scale, seed);
  std::vector<double> A = A0, V((size_t)r * r), t((size_t)r);
  const int sweeps = precond_jacobi(r, A.data(), V.data(), t.data());
  CHECK(sweeps < kPrecondJacobiSweeps);
  double norm = 0.0;
  for (double v : A0) norm += v * v;
  norm = std::sqrt(norm);
  const double eps = std::numeric_limits<double>::epsilon();
  double worst = 0.0, worst_orth = 0.0;
  for (int i = 0; i < r; ++i)
    for (int j = 0; j < r; ++j) {
      double rec = 0.0, dot = 0.0;
      for (int k = 0; k < r; ++k) rec += V[(size_t)i * r + k] * t[(size_t)k] * V[(size_t)j * r + k], dot += V[(size_t)k * r + i] * V[(size_t)k * r + j];
      worst = std::max(worst, std::fabs(rec - A0[(size_t)i * r + j]));
      worst_orth = std::max(worst_orth, std::fabs(dot - (i == j ? 1.0 : 0.0)));
    }
  CHECK(worst <= 64.0 * eps * r * norm);
  CHECK(worst_orth <= 64.0 * eps * r);
  for (int k = 0; k < r; ++k) CHECK(std::isfinite(t[(size_t)k]) && t[(size_t)k] >= -64.0 * eps * r * norm);
  // G and logdet P from it: symmetric, finite, zero in the padding; logdet against the sum over the eigenvalues
  const int rpad = precond_rpad(r);
  const double sigma2 = 1e-4;
  std::vector<double> G((size_t)rpad * rpad, -1.0);
  const PrecondSpectrum sp = precond_finish(1000, r, rpad, V.data(), t.data(), sigma2, G.data());
  CHECK(std::isfinite(sp.logdet_p) && sp.t_max >= 0.0);
  for (int i = 0; i < rpad; ++i)
    for (int j = 0; j < rpad; ++j) {
      const double g = G[(size_t)i * rpad + j];
      CHECK(std::isfinite(g) && g == G[(size_t)j * rpad + i]);
      if (i >= r || j >= r) CHECK(g == 0.0);
    }
}

static void check_g() {
  const double dmin = std::numeric_limits<double>::denorm_min();
  for (double sigma2 : {1e-6, 1e-2, 1.0, 1e3}) {
    ++g_cases;
    std::vector<double> ts = {0.0, dmin, 16 * dmin, std::numeric_limits<double>::min(), 1e-300, 1e-200, 1e-100, 1e-30};
    for (int e = -20; e <= 12; ++e) ts.push_back(std::pow(10.0, e) * sigma2);
    double prev = precond_g(0.0, sigma2);
    CHECK(prev == 0.5 / sigma2);
    CHECK(precond_g(-1e-9, sigma2) == prev);  // (a rounded zero eigenvalue counts as 0)
    for (double t : ts) {
      const double g = precond_g(t, sigma2);
      CHECK(std::isfinite(g) && g > 0.0 && g <= prev);
      // against the definition where it is well conditioned
      if (t >= 1e-3 * sigma2) CHECK(std::fabs(g - (1.0 - 1.0 / std::sqrt(1.0 + t / sigma2)) / t) <= 1e-12 * g);
      prev = g;
    }
  }
}

int main() {
  for (int64_t base : {0, 16, 32, 64, 128, 256, 1024, 4096, 16384, 262144})
    for (int64_t dn : {-17, -16, -15, -1, 0, 1, 15, 16, 17})
      for (int64_t cols = 1; cols <= 260; ++cols)
        for (int cus : {1, 64, 256}) {
          if (base + dn < 1) continue;
          check_slabs(base + dn, cols, cus);
        }
  for (int r : {1, 2, 5, 16, 33, 64, 128, 256}) {
    std::vector<double> ones((size_t)r, 1.0), decay((size_t)r), holes((size_t)r);
    for (int c = 0; c < r; ++c) decay[(size_t)c] = std::pow(10.0, -8.0 * c / std::max(r - 1, 1)), holes[(size_t)c] = c % 3 == 2 ? 0.0 : 1.0 / (1 + c);
    check_jacobi(r, 2 * r + 3, ones, 1u + r);     // full rank
    check_jacobi(r, r / 2 + 1, ones, 2u + r);     // rank-deficient
    check_jacobi(r, 2 * r + 3, decay, 3u + r);    // eigenvalues over 16 decades
    check_jacobi(r, 2 * r + 3, holes, 4u + r);    // zero columns: the Gram matrix of a factor that stopped early
  }
  check_g();
  printf("kernelprecond_check: %ld cases, %ld failed checks\n", g_cases, g_failed);
  return g_failed ? 1 : 0;
}
