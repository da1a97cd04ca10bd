// kernelgrad_check.cpp — the host part of csrc/slq_kernelgrad.hpp: kernel_grad_schedule() over sizes around the 16-point tile and
// the 128-row block, column counts around the 64-column chunk and several chip sizes, with what the kernel and the accumulator rely
// on checked on every answer (row blocks and slabs are partitions, slab bounds on tile boundaries, the kernel's own slab range from
// tiles_per_slab equals the schedule's, grids that fit the launch limits, a workgroup count that does not depend on m - the
// accumulator sizes its partials once -, the addition limit the tests' bar assumes). A stand-alone host program for the sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I primate_amd/csrc scripts/kernelgrad_check.cpp -o kernelgrad_check
//   ./kernelgrad_check
// It includes nothing but the header under test; no device, no library.
#include "slq_kernelgrad.hpp"

#include <vector>

using namespace slq;

static long g_cases = 0, g_failed = 0;
#define CHECK(cond)                                                                 \
  do {                                                                              \
    if (!(cond)) {                                                                  \
      if (g_failed++ < 20) fprintf(stderr, "case %ld: %s failed\n", g_cases, #cond); \
    }                                                                               \
  } while (0)

static void check_schedule(int64_t n, int m, int cus) {
  ++g_cases;
  const KernelGradSchedule S = kernel_grad_schedule(n, m, cus);
  CHECK(S.rows_per_block == kKernelRows && (int64_t)S.nrow_blocks * kKernelRows >= n && (int64_t)(S.nrow_blocks - 1) * kKernelRows < n);
  CHECK(S.chunk_cols == kKernelGradCols && (int64_t)S.ncol_chunks * S.chunk_cols >= m && (int64_t)(S.ncol_chunks - 1) * S.chunk_cols < m);
  CHECK(S.nslabs >= 1 && S.nslabs <= kKernelMaxSlabs && S.nslabs <= 65535);
  CHECK(S.slab_begin[0] == 0 && S.slab_begin[S.nslabs] == n);
  CHECK(S.nparts() == kernel_grad_schedule(n, 1, cus).nparts());  // (what slq_kernel_grad_create allocates for)
  const int64_t ntiles = kernel_npad(n) / 16;
  std::vector<int> owners((size_t)n, 0);
  for (int z = 0; z < S.nslabs; ++z) {
    CHECK(S.slab_begin[z] < S.slab_begin[z + 1] && S.slab_begin[z] % 16 == 0);
    int64_t t0, t1;
    kernel_slab_tiles<int64_t>(ntiles, S.tiles_per_slab, z, &t0, &t1);  // the kernel's range of slab z
    CHECK(std::min(n, t0 * 16) == S.slab_begin[z] && std::min(n, t1 * 16) == S.slab_begin[z + 1]);
    // no term passes through more than 2 n + 64 additions: the lane's run, 4 over lanes, 8 over waves, the partials
    CHECK((t1 - t0) * 16 + 4 + 8 + S.nparts() <= 2 * n + 64);
    for (int64_t j = S.slab_begin[z]; j < S.slab_begin[z + 1]; ++j) ++owners[(size_t)j];
  }
  CHECK((int64_t)S.nslabs * S.tiles_per_slab >= ntiles);
  for (int64_t j = 0; j < n; ++j) CHECK(owners[(size_t)j] == 1);
}

int main() {
  for (int64_t n : {1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 257, 1000, 4095, 20000, 262144})
    for (int m : {1, 3, 63, 64, 65, 128, 129, 1000})
      for (int cus : {1, 8, 255, 256, 304}) check_schedule(n, m, cus);
  printf("kernelgrad_check: %ld cases, %ld failed checks\n", g_cases, g_failed);
  return g_failed ? 1 : 0;
}
