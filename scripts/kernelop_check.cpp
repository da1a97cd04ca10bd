// kernelop_check.cpp — the host part of csrc/slq_kernelop.hpp: kernel_schedule() over sizes around the 16-point tile and the
// 128-row block at every panel shape and several chip sizes, with what the kernel relies on checked on every answer (row blocks
// and slabs are partitions, slab bounds on tile boundaries, the kernel's own slab range from tiles_per_slab equals the schedule's, the
// schedule equals kernel_cross_schedule(n, n, PW NP) wherever that one picks at most 16 slabs, a column-tile count the kernels are
// instantiated for, grids that fit the launch limits); kernel_validate() on damaged arguments - the first bad value is named; kernel_column_means() against a
// long-double sum. A stand-alone host program for the sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I primate_amd/csrc scripts/kernelop_check.cpp -o kernelop_check
//   ./kernelop_check
// It includes nothing but the header under test (and slq_kernelcross.hpp, for the schedule the operator's must agree with); no device,
// no library.
#include "slq_kernelcross.hpp"
#include "slq_kernelop.hpp"

#include <cstring>
#include <limits>
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

static void check_schedule(int64_t n, int PW, int NP, int cus) {
  ++g_cases;
  const KernelSchedule S = kernel_schedule(n, PW, NP, cus);
  CHECK(S.rows_per_block == kKernelRows && (int64_t)S.nrow_blocks * kKernelRows >= n && (int64_t)(S.nrow_blocks - 1) * kKernelRows < n);
  CHECK(S.col_blocks == 1 || S.col_blocks == 2 || S.col_blocks == 4 || S.col_blocks == 8 || S.col_blocks == 16);
  const int64_t ncols = (int64_t)PW * NP, per = 16 * S.col_blocks;
  CHECK((int64_t)S.ncol_chunks * per >= ncols && (int64_t)(S.ncol_chunks - 1) * per < ncols);
  CHECK(S.nslabs >= 1 && S.nslabs <= kKernelMaxSlabs && S.ncol_chunks <= 65535);
  CHECK(S.slab_begin[0] == 0 && S.slab_begin[S.nslabs] == n);
  std::vector<int> owners((size_t)n, 0);
  for (int z = 0; z < S.nslabs; ++z) {
    CHECK(S.slab_begin[z] < S.slab_begin[z + 1] && S.slab_begin[z] % 16 == 0);
    // the kernel's range of slab z, from tiles_per_slab, is the schedule's; and the split leaves no slack: cutting the tiles evenly
    // into nslabs gives the same tiles_per_slab
    const int64_t ntiles = kernel_npad(n) / 16, pt = (ntiles + S.nslabs - 1) / S.nslabs;
    CHECK(pt == S.tiles_per_slab && std::min(n, z * pt * 16) == S.slab_begin[z]);
    int64_t t0, t1;
    kernel_slab_tiles<int64_t>(ntiles, S.tiles_per_slab, z, &t0, &t1);
    CHECK(t0 < t1 && std::min(n, t0 * 16) == S.slab_begin[z] && std::min(n, t1 * 16) == S.slab_begin[z + 1]);
    int i0, i1;  // (as the device computes it: in int)
    kernel_slab_tiles<int>((int)ntiles, S.tiles_per_slab, z, &i0, &i1);
    CHECK(i0 == t0 && i1 == t1);
    for (int64_t j = S.slab_begin[z]; j < S.slab_begin[z + 1]; ++j) ++owners[(size_t)j];
  }
  for (int64_t j = 0; j < n; ++j) CHECK(owners[(size_t)j] == 1);
  // the operator's product is the cross product of the points with themselves, wherever that one stays within the operator's slab cap
  const KernelSchedule C = kernel_cross_schedule(n, n, ncols, cus);
  if (C.nslabs <= kKernelMaxSlabs) {
    CHECK(C.rows_per_block == S.rows_per_block && C.nrow_blocks == S.nrow_blocks && C.col_blocks == S.col_blocks && C.ncol_chunks == S.ncol_chunks);
    CHECK(C.nslabs == S.nslabs && C.tiles_per_slab == S.tiles_per_slab);
    for (int z = 0; z <= kKernelCrossMaxSlabs; ++z) CHECK(C.slab_begin[z] == S.slab_begin[z]);
  }
}

int main() {
  for (int64_t n : {1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 257, 1000, 4095, 20000, 262144})
    for (int PW : {16, 32, 64, 128, 256})
      for (int NP : {1, 2, 3, 7})
        for (int cus : {1, 8, 255, 256, 304}) check_schedule(n, PW, NP, cus);
  CHECK(kernel_dpad(1) == 4 && kernel_dpad(4) == 4 && kernel_dpad(5) == 8 && kernel_dpad(64) == 64 && kernel_npad(1) == 16 && kernel_npad(16) == 16 && kernel_npad(17) == 32);

  // validation: the first bad value is named
  std::mt19937_64 rng(7);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  const int64_t n = 37;
  const int d = 5, ldp = 7;
  std::vector<double> X((size_t)n * ldp);
  for (double &v : X) v = U(rng);
  std::vector<float> Xf(X.begin(), X.end());
  const double ls1[1] = {0.5}, ls5[5] = {1, 2, 3, 4, 5};
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  char msg[256];
  auto what = [&](const KernelBad &b) { ++g_cases; kernel_bad_message(b, msg, sizeof msg); CHECK(strlen(msg) > 10); return b.what; };
  CHECK(what(kernel_validate<double>(n, d, X.data(), ldp, KERNEL_RBF, ls1, 1, 1.0, 0.0)) == KERNEL_OK);
  CHECK(what(kernel_validate<float>(n, d, Xf.data(), ldp, KERNEL_MATERN52, ls5, 5, 2.0, 0.1)) == KERNEL_OK);
  CHECK(what(kernel_validate<double>(n, d, nullptr, ldp, KERNEL_RBF, ls1, 1, 1.0, 0.0)) == KERNEL_OK);  // (points on the device: not read)
  CHECK(what(kernel_validate<double>(0, d, X.data(), ldp, 0, ls1, 1, 1.0, 0.0)) == KERNEL_BAD_N);
  CHECK(what(kernel_validate<double>((int64_t)1 << 31, d, nullptr, ldp, 0, ls1, 1, 1.0, 0.0)) == KERNEL_BAD_N);
  CHECK(what(kernel_validate<double>(n, 0, X.data(), ldp, 0, ls1, 1, 1.0, 0.0)) == KERNEL_BAD_DIM);
  CHECK(what(kernel_validate<double>(n, 65, X.data(), 65, 0, ls1, 1, 1.0, 0.0)) == KERNEL_BAD_DIM);
  CHECK(what(kernel_validate<double>(n, d, X.data(), 4, 0, ls1, 1, 1.0, 0.0)) == KERNEL_BAD_LDP);
  CHECK(what(kernel_validate<double>(n, d, X.data(), ldp, 4, ls1, 1, 1.0, 0.0)) == KERNEL_BAD_PROFILE);
  CHECK(what(kernel_validate<double>(n, d, X.data(), ldp, -1, ls1, 1, 1.0, 0.0)) == KERNEL_BAD_PROFILE);
  CHECK(what(kernel_validate<double>(n, d, X.data(), ldp, 0, ls5, 3, 1.0, 0.0)) == KERNEL_BAD_NLS);
  CHECK(what(kernel_validate<double>(n, d, X.data(), ldp, 0, nullptr, 1, 1.0, 0.0)) == KERNEL_BAD_NLS);
  for (double badv : {0.0, -1.0, nan, inf}) {
    double l[5] = {1, 2, badv, 4, badv};
    const KernelBad b = kernel_validate<double>(n, d, X.data(), ldp, 0, l, 5, 1.0, 0.0);
    CHECK(what(b) == KERNEL_BAD_LENGTHSCALE && b.row == 2);
    CHECK(what(kernel_validate<double>(n, d, X.data(), ldp, 0, ls1, 1, badv, 0.0)) == KERNEL_BAD_OUTPUTSCALE);
  }
  for (double badv : {-1e-300, nan, inf}) CHECK(what(kernel_validate<double>(n, d, X.data(), ldp, 0, ls1, 1, 1.0, badv)) == KERNEL_BAD_NOISE);
  CHECK(what(kernel_validate_parameters(d, ls5, 5, 1.0, 0.0)) == KERNEL_OK);
  {
    std::vector<double> B = X;
    B[(size_t)20 * ldp + 3] = inf, B[(size_t)11 * ldp + 4] = nan, B[(size_t)11 * ldp + 6] = nan;  // (column 6 is padding: never read)
    B[(size_t)3 * ldp + 5] = nan;
    const KernelBad b = kernel_validate<double>(n, d, B.data(), ldp, 0, ls1, 1, 1.0, 0.0);
    CHECK(what(b) == KERNEL_BAD_POINT && b.row == 11 && b.col == 4);
    CHECK(strstr(msg, "point 11, coordinate 4") != nullptr);
    std::vector<float> Bf(B.begin(), B.end());
    const KernelBad bf = kernel_validate<float>(n, d, Bf.data(), ldp, 0, ls1, 1, 1.0, 0.0);
    CHECK(what(bf) == KERNEL_BAD_POINT && bf.row == 11 && bf.col == 4);
  }
  // the centre
  {
    ++g_cases;
    double mean[kKernelMaxDim];
    kernel_column_means<double>(n, d, X.data(), ldp, mean);
    for (int k = 0; k < d; ++k) {
      long double s = 0.0L;
      for (int64_t i = 0; i < n; ++i) s += X[(size_t)i * ldp + k];
      CHECK(std::fabs((double)(s / n) - mean[k]) <= 1e-15);
    }
    float meanf_src[3] = {1e4f, 1e4f + 1.0f, 1e4f + 2.0f};
    kernel_column_means<float>(3, 1, meanf_src, 1, mean);
    CHECK(mean[0] == 1e4 + 1.0);
  }
  printf("kernelop_check: %ld cases, %ld failed checks\n", g_cases, g_failed);
  return g_failed ? 1 : 0;
}
