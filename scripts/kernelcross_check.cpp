// kernelcross_check.cpp — the host part of csrc/slq_kernelcross.hpp: kernel_cross_schedule() over row counts and summed counts
// around the 16-point tile and the 128-row block, column counts around the 16-column tile and the 256-column chunk and several chip
// sizes, with what the kernel and the C-ABI rely on checked on every answer (row blocks and slabs are partitions of whole tiles, no
// slab is empty, the kernel's own slab range from tiles_per_slab equals the schedule's, the column tiles cover min(b, 256) with the
// smallest of 1, 2, 4, 8, 16, the chunks cover b, the slab count stays under its cap). A stand-alone host program for the sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I primate_amd/csrc scripts/kernelcross_check.cpp -o kernelcross_check
//   ./kernelcross_check
// It includes nothing but the header under test; no device, no library.
#include "slq_kernelcross.hpp"

#include <vector>

using namespace slq;

static long g_cases = 0, g_failed = 0;
#define CHECK(cond)                                                                 \
  do {                                                                              \
    if (!(cond)) {                                                                  \
      if (g_failed++ < 20) fprintf(stderr, "case %ld: %s failed\n", g_cases, #cond); \
    }                                                                               \
  } while (0)

static void check_schedule(int64_t nrows, int64_t nsum, int64_t b, int cus) {
  ++g_cases;
  const KernelSchedule S = kernel_cross_schedule(nrows, nsum, b, cus);
  CHECK(S.rows_per_block == kKernelRows && (int64_t)S.nrow_blocks * kKernelRows >= nrows && (int64_t)(S.nrow_blocks - 1) * kKernelRows < nrows);
  const int64_t first = std::min<int64_t>(b, 256);
  CHECK(S.col_blocks == 1 || S.col_blocks == 2 || S.col_blocks == 4 || S.col_blocks == 8 || S.col_blocks == 16);
  CHECK(16 * S.col_blocks >= first && (S.col_blocks == 1 || 16 * (S.col_blocks / 2) < first));
  CHECK((int64_t)S.ncol_chunks * 256 >= b && (int64_t)(S.ncol_chunks - 1) * 256 < b);
  CHECK(S.ncol_chunks == 1 || S.col_blocks == 16);  // (a workgroup of a later chunk starts at column 256 y)
  CHECK(S.nslabs >= 1 && S.nslabs <= kKernelCrossMaxSlabs);
  CHECK(S.slab_begin[0] == 0 && S.slab_begin[S.nslabs] == nsum);
  const int64_t ntiles = kernel_npad(nsum) / 16;
  std::vector<int> owners((size_t)nsum, 0);
  for (int z = 0; z < S.nslabs; ++z) {
    CHECK(S.slab_begin[z] < S.slab_begin[z + 1] && S.slab_begin[z] % 16 == 0);
    int64_t t0, t1;
    kernel_slab_tiles<int64_t>(ntiles, S.tiles_per_slab, z, &t0, &t1);  // the kernel's range of slab z
    CHECK(t0 < t1 && std::min(nsum, t0 * 16) == S.slab_begin[z] && std::min(nsum, t1 * 16) == S.slab_begin[z + 1]);
    for (int64_t j = S.slab_begin[z]; j < S.slab_begin[z + 1]; ++j) ++owners[(size_t)j];
  }
  CHECK((int64_t)S.nslabs * S.tiles_per_slab >= ntiles);
  for (int64_t j = 0; j < nsum; ++j) CHECK(owners[(size_t)j] == 1);
}

int main() {
  const int64_t sizes[] = {1, 2, 15, 16, 17, 31, 33, 127, 128, 129, 255, 257, 1000, 1023, 1025, 4095, 16384, 20000};
  for (int64_t nrows : sizes)
    for (int64_t nsum : sizes)
      for (int64_t b : {1, 3, 15, 16, 17, 64, 65, 128, 255, 256, 257, 260, 1000})
        for (int cus : {1, 8, 255, 256, 304}) check_schedule(nrows, nsum, b, cus);
  check_schedule(128, 262144, 1, 256);
  check_schedule(262144, 128, 128, 256);
  printf("kernelcross_check: %ld cases, %ld failed checks\n", g_cases, g_failed);
  return g_failed ? 1 : 0;
}
