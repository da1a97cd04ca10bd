// kernelfeatureadj_check.cpp — the host part of csrc/slq_kernelfeatureadj.hpp: kernel_feature_adjoint_schedule() for every shape of
// the adjoint tests' table (rows = the operator's points and the 1, 40 and 130 new points of the cross form, and the seventh cell of
// 2000 points against one row block of 40 frequencies, which takes many slabs), around the 16-point tile, the 128-frequency row block,
// the 128-column chunk of fp64 and the 256-column chunk of fp32, on several chip sizes, with what the kernel and the C-ABI rely on
// checked on every answer: row blocks of the frequencies and slabs of the row points are partitions of whole tiles, no slab is
// empty, the kernel's own slab range from tiles_per_slab equals the schedule's, the column tiles are the smallest of 1, 2, 4, 8, 16
// that cover the first chunk, fp64 never asks for 16, the chunks cover b. A stand-alone host program for the sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I primate_amd/csrc scripts/kernelfeatureadj_check.cpp -o kernelfeatureadj_check
//   ./kernelfeatureadj_check
// It includes nothing but the header under test; no device, no library.
#include "slq_kernelfeatureadj.hpp"

#include <vector>

using namespace slq;

static long g_cases = 0, g_failed = 0;
#define CHECK(cond)                                                                 \
  do {                                                                              \
    if (!(cond)) {                                                                  \
      if (g_failed++ < 20) fprintf(stderr, "case %ld: %s failed\n", g_cases, #cond); \
    }                                                                               \
  } while (0)

static KernelSchedule check_schedule(int64_t f2, int64_t nrows, int64_t b, int cus, bool f64) {
  ++g_cases;
  const KernelSchedule S = kernel_feature_adjoint_schedule(f2, nrows, b, cus, f64);
  const int chunk = kernel_feature_adjoint_chunk_cols(f64);
  CHECK(chunk == (f64 ? 128 : 256));
  CHECK(S.rows_per_block == kKernelRows && (int64_t)S.nrow_blocks * kKernelRows >= f2 && (int64_t)(S.nrow_blocks - 1) * kKernelRows < f2);
  const int64_t first = std::min<int64_t>(b, chunk);
  CHECK(S.col_blocks == 1 || S.col_blocks == 2 || S.col_blocks == 4 || S.col_blocks == 8 || S.col_blocks == 16);
  CHECK(!f64 || S.col_blocks <= kKernelFeatureAdjMaxColBlocksF64);
  CHECK(16 * S.col_blocks >= first && (S.col_blocks == 1 || 16 * (S.col_blocks / 2) < first));
  CHECK((int64_t)S.ncol_chunks * chunk >= b && (int64_t)(S.ncol_chunks - 1) * chunk < b);
  CHECK(S.ncol_chunks == 1 || 16 * S.col_blocks == chunk);  // (a workgroup of a later chunk starts at column chunk * y)
  CHECK(S.nslabs >= 1 && S.nslabs <= kKernelCrossMaxSlabs);
  CHECK(S.slab_begin[0] == 0 && S.slab_begin[S.nslabs] == nrows);
  const int64_t ntiles = kernel_npad(nrows) / 16;
  std::vector<int> owners((size_t)nrows, 0);
  for (int z = 0; z < S.nslabs; ++z) {
    CHECK(S.slab_begin[z] < S.slab_begin[z + 1] && S.slab_begin[z] % 16 == 0);
    int64_t t0, t1;
    kernel_slab_tiles<int64_t>(ntiles, S.tiles_per_slab, z, &t0, &t1);  // the kernel's range of slab z
    CHECK(t0 < t1 && std::min(nrows, t0 * 16) == S.slab_begin[z] && std::min(nrows, t1 * 16) == S.slab_begin[z + 1]);
    for (int64_t i = S.slab_begin[z]; i < S.slab_begin[z + 1]; ++i) ++owners[(size_t)i];
  }
  CHECK((int64_t)S.nslabs * S.tiles_per_slab >= ntiles);
  for (int64_t i = 0; i < nrows; ++i) CHECK(owners[(size_t)i] == 1);
  // the row blocks: every frequency in exactly one block of kKernelRows
  std::vector<int> rows((size_t)f2, 0);
  for (int rb = 0; rb < S.nrow_blocks; ++rb)
    for (int64_t j = (int64_t)rb * kKernelRows; j < std::min<int64_t>(f2, (int64_t)(rb + 1) * kKernelRows); ++j) ++rows[(size_t)j];
  for (int64_t j = 0; j < f2; ++j) CHECK(rows[(size_t)j] == 1);
  // the column chunks: every column in exactly one chunk
  std::vector<int> cols((size_t)b, 0);
  for (int cy = 0; cy < S.ncol_chunks; ++cy)
    for (int64_t g = (int64_t)cy * chunk; g < std::min<int64_t>(b, (int64_t)cy * chunk + 16 * S.col_blocks); ++g) ++cols[(size_t)g];
  for (int64_t g = 0; g < b; ++g) CHECK(cols[(size_t)g] == 1);
  return S;
}

int main() {
  // the table of tests/_kernelfeatureadj_ref.py: (n, F2, b), and the new points of the cross form for the first six
  const int64_t table[][3] = {{1, 1, 1}, {17, 16, 1}, {130, 33, 5}, {257, 500, 260}, {300, 1024, 16}, {129, 100, 17}, {2000, 40, 3}};
  int idx = 0;
  for (const auto &t : table) {
    for (int64_t rows : {t[0], (int64_t)1, (int64_t)40, (int64_t)130}) {
      if (idx == 6 && rows != t[0]) continue;
      for (int cus : {1, 8, 255, 256, 304})
        for (bool f64 : {false, true}) check_schedule(t[1], rows, t[2], cus, f64);
    }
    ++idx;
  }
  // one row block of frequencies against many points: the chip is fed by slabs
  for (bool f64 : {false, true}) {
    const KernelSchedule S = check_schedule(40, 2000, 3, 256, f64);
    CHECK(S.nrow_blocks == 1 && S.nslabs > 8);
    const KernelSchedule B = check_schedule(1024, 16384, 64, 256, f64);  // the benchmark's shape: 8 row blocks
    CHECK(B.nrow_blocks == 8 && B.ncol_chunks == 1 && B.nslabs > 1);
  }
  const int64_t sizes[] = {1, 2, 15, 16, 17, 31, 33, 127, 128, 129, 255, 257, 1000, 1025, 4096, 16384};
  for (int64_t f2 : sizes)
    for (int64_t nrows : sizes)
      for (int64_t b : {1, 3, 16, 17, 64, 65, 127, 128, 129, 255, 256, 257, 260, 512, 1000})
        for (int cus : {1, 256, 304})
          for (bool f64 : {false, true}) check_schedule(f2, nrows, b, cus, f64);
  check_schedule(4096, 65536, 64, 256, true);
  check_schedule(128, 1 << 20, 1, 256, false);
  printf("kernelfeatureadj_check: %ld cases, %ld failed checks\n", g_cases, g_failed);
  return g_failed ? 1 : 0;
}
