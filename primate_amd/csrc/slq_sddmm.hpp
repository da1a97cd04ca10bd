// slq_sddmm.hpp — the sampled dense-dense product on a CSR pattern (slq_sddmm_*): for every stored nonzero e = (r, c)
//   vals[e] = beta * vals[e] + alpha * sum_{j < m} W[r, j] * Z[c, j]
// over two tall-skinny column-major matrices (slq_dmat, ld = n): the Hutchinson estimate of d tr f(A) / dA = f'(A) on the
// stored nonzeros, with W = f'(A) V and Z = V (primate_amd.grad).
// Two parts:
//   sddmm_schedule   plain C++ (no HIP include, no HIP call; it runs without a device - slq_debug_sddmm_schedule,
//                    tests/test_sddmm_cpu.py): the pattern's rows cut into work items, one wave each. A short item is a run
//                    of at most 64 consecutive rows of at most kSddmmLongRow nonzeros inside one aligned block of 64 rows,
//                    one lane per row; a long item is one row of more nonzeros, the lanes over its nonzeros. Every stored
//                    nonzero belongs to exactly one item; runs without a nonzero make no item, so nnz = 0 launches nothing.
//   k_sddmm          the kernel the items drive (compiled by hipcc only). A lane owns its nonzeros outright and sums j
//                    ascending into a register: no float atomics, no cross-lane reduction, identical calls give identical
//                    bits. W and Z are only read, so they may be the same matrix.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

namespace slq {

constexpr int kSddmmLongRow = 64;  // a row of more nonzeros than this takes a wave of its own
constexpr int kSddmmChunk = 8;     // nonzeros a lane carries in registers through one sweep over j
constexpr int kSddmmWaves = 4;     // items (waves) per workgroup

struct SddmmItem {
  int32_t row0;   // first row
  int32_t nrows;  // short item: rows row0 .. row0 + nrows - 1, one lane each; 0: the long row row0
};

struct SddmmSchedule {
  std::vector<SddmmItem> items;
  int64_t nlong = 0;  // long rows among them
  int64_t grid = 0;   // workgroups of kSddmmWaves waves
};

// rowptr: n + 1 non-decreasing offsets starting at 0 (the caller has checked them).
inline SddmmSchedule sddmm_schedule(int64_t n, const int32_t *rowptr) {
  SddmmSchedule S;
  for (int64_t b = 0; b < n; b += 64) {
    const int64_t bend = std::min<int64_t>(n, b + 64);
    int64_t r = b;
    while (r < bend) {
      if (rowptr[r + 1] - rowptr[r] > kSddmmLongRow) {
        S.items.push_back(SddmmItem{(int32_t)r, 0});
        ++S.nlong;
        ++r;
        continue;
      }
      int64_t q = r;
      while (q < bend && rowptr[q + 1] - rowptr[q] <= kSddmmLongRow) ++q;
      if (rowptr[q] > rowptr[r]) S.items.push_back(SddmmItem{(int32_t)r, (int32_t)(q - r)});
      r = q;
    }
  }
  S.grid = ((int64_t)S.items.size() + kSddmmWaves - 1) / kSddmmWaves;
  return S;
}

// The nonzeros item `it` owns: [e0, e1), contiguous in the caller's order.
inline void sddmm_item_range(const SddmmItem &it, const int32_t *rowptr, int64_t *e0, int64_t *e1) {
  *e0 = rowptr[it.row0];
  *e1 = rowptr[it.row0 + (it.nrows ? it.nrows : 1)];
}

// First row at which (rowptr, colind) is not a CSR pattern over n rows and columns with nnz entries, or -1: rowptr[0] == 0,
// rowptr non-decreasing and never above nnz, 0 <= colind < n, rowptr[n] == nnz (reported at row n). colind is read only
// inside offsets already checked.
inline int64_t sddmm_first_bad_row(int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colind) {
  if (rowptr[0] != 0) return 0;
  for (int64_t i = 0; i < n; ++i) {
    if (rowptr[i + 1] < rowptr[i] || (int64_t)rowptr[i + 1] > nnz) return i;
    for (int32_t q = rowptr[i]; q < rowptr[i + 1]; ++q)
      if (colind[q] < 0 || (int64_t)colind[q] >= n) return i;
  }
  return rowptr[n] == nnz ? -1 : n;
}

#ifdef __HIPCC__
// One wave per item. Short item: lane l owns row row0 + l and takes its nonzeros kSddmmChunk at a time; W[r, j] is one
// coalesced load per j, Z[colind, j] the gather of the generic CSR product. Long item: lane l owns the nonzeros
// rowptr[r] + l + 64 t of the one row, kSddmmChunk of them at a time (colind coalesced, W[r, j] the same word for the wave).
// A slot past the row's end gathers the lane's own row (a valid address) and is not stored. SYM: the summand is
// W[r,j] Z[c,j] + Z[r,j] W[c,j] and the host passes alpha / 2. beta == 0 does not read vals.
template <bool SYM>
__global__ __launch_bounds__(64 * kSddmmWaves) void k_sddmm(int64_t nitems, const SddmmItem *__restrict__ items, const int32_t *__restrict__ rowptr,
                                                            const int32_t *__restrict__ colind, int64_t ld, const double *W, const double *Z, int m,
                                                            double alpha, double beta, double *__restrict__ vals) {
  const int lane = threadIdx.x & 63;
  const int64_t it = (int64_t)blockIdx.x * kSddmmWaves + (threadIdx.x >> 6);
  if (it >= nitems) return;
  const SddmmItem item = items[it];
  const bool longrow = item.nrows == 0;
  if (!longrow && lane >= item.nrows) return;
  const int64_t r = (int64_t)item.row0 + (longrow ? 0 : lane);
  const int64_t stride = longrow ? 64 : 1;
  const int64_t end = rowptr[r + 1];
  for (int64_t e = (int64_t)rowptr[r] + (longrow ? lane : 0); e < end; e += kSddmmChunk * stride) {
    int64_t c[kSddmmChunk];
    double acc[kSddmmChunk];
#pragma unroll
    for (int k = 0; k < kSddmmChunk; ++k) {
      const int64_t q = e + k * stride;
      c[k] = q < end ? (int64_t)colind[q] : r;
      acc[k] = 0.0;
    }
    const double *wj = W, *zj = Z;
    for (int j = 0; j < m; ++j, wj += ld, zj += ld) {
      const double w = wj[r];
      if (SYM) {
        const double z = zj[r];
#pragma unroll
        for (int k = 0; k < kSddmmChunk; ++k) acc[k] = fma(z, wj[c[k]], fma(w, zj[c[k]], acc[k]));
      } else {
#pragma unroll
        for (int k = 0; k < kSddmmChunk; ++k) acc[k] = fma(w, zj[c[k]], acc[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < kSddmmChunk; ++k) {
      const int64_t q = e + k * stride;
      if (q < end) vals[q] = beta == 0.0 ? alpha * acc[k] : fma(beta, vals[q], alpha * acc[k]);
    }
  }
}
#endif  // __HIPCC__

}  // namespace slq
