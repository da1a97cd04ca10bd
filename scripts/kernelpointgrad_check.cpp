// kernelpointgrad_check.cpp — the host part of csrc/slq_kernelpointgrad.hpp: kernel_pointgrad_schedule() over row and summed point
// counts around the 16-point tile and the 128-row block and several chip sizes, with what the kernel and the accumulator rely on
// checked on every answer (row blocks and slabs are partitions, slab bounds on tile boundaries, the kernel's own slab range from
// tiles_per_slab equals the schedule's, grids that fit the launch limits, a partial buffer of nslabs x nrows x dpad words that fits an
// int64 index, the addition limit the tests' bar assumes). A stand-alone host program for the sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I primate_amd/csrc scripts/kernelpointgrad_check.cpp -o kernelpointgrad_check
//   ./kernelpointgrad_check
// It includes nothing but the header under test; no device, no library.
#include "slq_kernelpointgrad.hpp"

#include <cstdio>
#include <vector>

using namespace slq;

static long g_cases = 0, g_failed = 0;
#define CHECK(cond)                                                                 \
  do {                                                                              \
    if (!(cond)) {                                                                  \
      if (g_failed++ < 20) fprintf(stderr, "case %ld: %s failed\n", g_cases, #cond); \
    }                                                                               \
  } while (0)

static void check_schedule(int64_t nrows, int64_t nsum, int cus) {
  ++g_cases;
  const KernelPointGradSchedule S = kernel_pointgrad_schedule(nrows, nsum, cus);
  CHECK(S.rows_per_block == kKernelRows && (int64_t)S.nrow_blocks * kKernelRows >= nrows && (int64_t)(S.nrow_blocks - 1) * kKernelRows < nrows);
  CHECK(S.chunk_cols == kKernelPointGradCols);
  CHECK(S.nslabs >= 1 && S.nslabs <= kKernelCrossMaxSlabs && S.nslabs <= 65535);
  CHECK(S.slab_begin[0] == 0 && S.slab_begin[S.nslabs] == nsum);
  const int64_t ntiles = (nsum + 15) / 16;
  std::vector<int> owners((size_t)nsum, 0);
  for (int z = 0; z < S.nslabs; ++z) {
    CHECK(S.slab_begin[z] < S.slab_begin[z + 1] && S.slab_begin[z] % 16 == 0);
    int64_t t0, t1;
    kernel_slab_tiles<int64_t>(ntiles, S.tiles_per_slab, z, &t0, &t1);  // the kernel's range of slab z
    CHECK(std::min(nsum, t0 * 16) == S.slab_begin[z] && std::min(nsum, t1 * 16) == S.slab_begin[z + 1]);
    // no term passes through more than nsum + 80 additions: the lane's run over the slab's padded points, the slabs, the two folds
    CHECK((t1 - t0) * 16 + (S.nslabs - 1) + 2 <= nsum + 80);
    for (int64_t j = S.slab_begin[z]; j < S.slab_begin[z + 1]; ++j) ++owners[(size_t)j];
  }
  CHECK((int64_t)S.nslabs * S.tiles_per_slab >= ntiles);
  for (int64_t j = 0; j < nsum; ++j) CHECK(owners[(size_t)j] == 1);
  // the partials: nslabs x nrows x dpad words at the deepest dpad
  CHECK((double)S.nslabs * (double)nrows * kKernelMaxDim * 8.0 < 9.0e18);
}

int main() {
  for (int64_t nrows : {1, 2, 15, 16, 17, 127, 128, 129, 257, 1000, 4095, 20000, 262144})
    for (int64_t nsum : {1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 257, 1000, 4095, 20000, 262144})
      for (int cus : {1, 8, 255, 256, 304}) check_schedule(nrows, nsum, cus);
  printf("kernelpointgrad_check: %ld cases, %ld failed checks\n", g_cases, g_failed);
  return g_failed ? 1 : 0;
}
