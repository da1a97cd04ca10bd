// kernelfeature_check.cpp — the host part of csrc/slq_kernelfeature.hpp: kernel_feature_schedule() for every shape of the feature
// tests' table (rows = the operator's points and the 1, 40 and 130 new points of the cross form, among them the one-row-block case of
// m = 40 that takes many slabs), around the 16-frequency tile, the 128-row block, the 128-column chunk of fp64 and the 256-column
// chunk of fp32, on several chip sizes, with what the kernel and the C-ABI rely on checked on every answer: row blocks and frequency
// slabs are partitions of whole tiles, no slab is empty, the kernel's own slab range from tiles_per_slab equals the schedule's, the
// column tiles are the smallest of 1, 2, 4, 8, 16 that cover the first chunk, fp64 never asks for 16, the chunks cover b. A
// stand-alone host program for the sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I primate_amd/csrc scripts/kernelfeature_check.cpp -o kernelfeature_check
//   ./kernelfeature_check
// It includes nothing but the header under test; no device, no library.
#include "slq_kernelfeature.hpp"

#include <vector>

using namespace slq;

static long g_cases = 0, g_failed = 0;
#define CHECK(cond)                                                                 \
  do {                                                                              \
    if (!(cond)) {                                                                  \
      if (g_failed++ < 20) fprintf(stderr, "case %ld: %s failed\n", g_cases, #cond); \
    }                                                                               \
  } while (0)

static KernelSchedule check_schedule(int64_t nrows, int64_t f2, int64_t b, int cus, bool f64) {
  ++g_cases;
  const KernelSchedule S = kernel_feature_schedule(nrows, f2, b, cus, f64);
  const int chunk = kernel_feature_chunk_cols(f64);
  CHECK(chunk == (f64 ? 128 : 256));
  CHECK(S.rows_per_block == kKernelRows && (int64_t)S.nrow_blocks * kKernelRows >= nrows && (int64_t)(S.nrow_blocks - 1) * kKernelRows < nrows);
  const int64_t first = std::min<int64_t>(b, chunk);
  CHECK(S.col_blocks == 1 || S.col_blocks == 2 || S.col_blocks == 4 || S.col_blocks == 8 || S.col_blocks == 16);
  CHECK(!f64 || S.col_blocks <= kKernelFeatureMaxColBlocksF64);
  CHECK(16 * S.col_blocks >= first && (S.col_blocks == 1 || 16 * (S.col_blocks / 2) < first));
  CHECK((int64_t)S.ncol_chunks * chunk >= b && (int64_t)(S.ncol_chunks - 1) * chunk < b);
  CHECK(S.ncol_chunks == 1 || 16 * S.col_blocks == chunk);  // (a workgroup of a later chunk starts at column chunk * y)
  CHECK(S.nslabs >= 1 && S.nslabs <= kKernelCrossMaxSlabs);
  CHECK(S.slab_begin[0] == 0 && S.slab_begin[S.nslabs] == f2);
  const int64_t ntiles = kernel_npad(f2) / 16;
  std::vector<int> owners((size_t)f2, 0);
  for (int z = 0; z < S.nslabs; ++z) {
    CHECK(S.slab_begin[z] < S.slab_begin[z + 1] && S.slab_begin[z] % 16 == 0);
    int64_t t0, t1;
    kernel_slab_tiles<int64_t>(ntiles, S.tiles_per_slab, z, &t0, &t1);  // the kernel's range of slab z
    CHECK(t0 < t1 && std::min(f2, t0 * 16) == S.slab_begin[z] && std::min(f2, t1 * 16) == S.slab_begin[z + 1]);
    for (int64_t j = S.slab_begin[z]; j < S.slab_begin[z + 1]; ++j) ++owners[(size_t)j];
  }
  CHECK((int64_t)S.nslabs * S.tiles_per_slab >= ntiles);
  for (int64_t j = 0; j < f2; ++j) CHECK(owners[(size_t)j] == 1);
  // the row blocks: every row in exactly one block of kKernelRows
  std::vector<int> rows((size_t)nrows, 0);
  for (int rb = 0; rb < S.nrow_blocks; ++rb)
    for (int64_t i = (int64_t)rb * kKernelRows; i < std::min<int64_t>(nrows, (int64_t)(rb + 1) * kKernelRows); ++i) ++rows[(size_t)i];
  for (int64_t i = 0; i < nrows; ++i) CHECK(rows[(size_t)i] == 1);
  return S;
}

int main() {
  // the table of tests/_kernelfeature_ref.py: (n, F2, b), and the new points of the cross form
  const int64_t table[][3] = {{1, 1, 1}, {17, 16, 1}, {130, 33, 5}, {257, 500, 260}, {300, 1024, 16}, {129, 100, 17}};
  for (const auto &t : table)
    for (int64_t rows : {t[0], (int64_t)1, (int64_t)40, (int64_t)130})
      for (int cus : {1, 8, 255, 256, 304})
        for (bool f64 : {false, true}) check_schedule(rows, t[1], t[2], cus, f64);
  // one row block against many frequencies: the chip is fed by slabs
  for (bool f64 : {false, true}) {
    const KernelSchedule S = check_schedule(40, 1024, 16, 256, f64);
    CHECK(S.nrow_blocks == 1 && S.nslabs > 8);
  }
  const int64_t sizes[] = {1, 2, 15, 16, 17, 31, 33, 127, 128, 129, 255, 257, 1000, 1025, 4096, 16384};
  for (int64_t nrows : sizes)
    for (int64_t f2 : sizes)
      for (int64_t b : {1, 3, 16, 17, 64, 65, 127, 128, 129, 255, 256, 257, 260, 512, 1000})
        for (int cus : {1, 256, 304})
          for (bool f64 : {false, true}) check_schedule(nrows, f2, b, cus, f64);
  check_schedule(65536, 4096, 64, 256, true);
  check_schedule(128, 1 << 20, 1, 256, false);
  printf("kernelfeature_check: %ld cases, %ld failed checks\n", g_cases, g_failed);
  return g_failed ? 1 : 0;
}
