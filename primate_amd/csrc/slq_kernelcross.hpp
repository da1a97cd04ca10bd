// slq_kernelcross.hpp — cross-covariance products of the matrix-free kernel operator (slq_kernel_cross_*). For a
// kernel operator with points x_1..x_n (centre mean(x), lengthscales l, outputscale s, dtype F) and m NEW points x*_1..x*_m
//   z*_i = (F)(((double)x*_i - mean(x)) / l)        the TRAINING centre, double arithmetic, one rounding
//   r2_ij = max(0, fma(-2, z*_i.z_j, |z*_i|^2 + |z_j|^2))        no diagonal rule
//   C = s phi(r2)        m x n, no noise term
// and the two products Y = C W (forward: W n x b, Y m x b) and Y = C^T U (adjoint: U m x b, Y n x b). Both are ONE kernel with the
// two point sets exchanging roles: the "row" points own the output rows, the "summed" points are walked in tiles of 16. C is
// never held. The tile walk, the product kernel, the profiles and the slab rule are those of slq_kerneltile.hpp; here is what is the
// cross product's own:
//   host (plain C++, no HIP include; scripts/kernelcross_check.cpp runs it under the host sanitizers)
//     kernel_cross_schedule   row blocks, column chunks and slabs of the summed points for (nrows, nsum, b, num_cus)
//                             (slq_debug_kernel_cross_schedule)
//   device (hipcc only)
//     k_kernel_cross       Y (or one slab's partial of it) = s phi(r2) W on column-major operands with a leading dimension:
//                          kernel_product on KernelColumnLayout
//     k_kernel_cross_sum   the slab partials summed in slab order
//   The instantiations of k_kernel_cross (2 dtypes x 4 profiles x 5 NCB x 2 DQ) live in slq_kernelcross.hip, a translation unit
//   of their own; slq.hip sees only kernel_cross_launch / kernel_cross_sum_launch.
#pragma once

#include "slq_kernelop.hpp"

namespace slq {

// ---- the schedule of one product ------------------------------------------------------------------------------------------
// kernel_product_schedule (slq_kerneltile.hpp) for nrows row points, nsum summed points and b columns. Few rows (a forward product
// with m = 128 new points is ONE row block): up to kKernelCrossMaxSlabs slabs; slab z lands in its own partial and the partials
// are summed in slab order by k_kernel_cross_sum. One slab writes the result directly.
inline KernelSchedule kernel_cross_schedule(int64_t nrows, int64_t nsum, int64_t b, int num_cus) {
  return kernel_product_schedule(nrows, nsum, b, num_cus, kKernelCrossMaxSlabs);
}

// what a launch reads and writes (plain pointers: the launch functions are defined in slq_kernelcross.hip and called from slq.hip)
struct KernelCrossArgs {
  int nrows, rpad;  // row points: count, count rounded up to 16
  int nsum, spad;   // summed points
  int dq;           // dpad / 4
  const void *rzt, *rnrm;  // row points: z transposed (dpad x rpad), |z|^2 (rpad)
  const void *szt, *snrm;  // summed points
  const void *params;      // {s, sigma2} of the operator, on the device; only s is read
  const void *W;           // nsum x b, column-major
  int64_t ldw;
  int b;
  void *out;  // nslabs == 1: Y (nrows x b, column-major, ldo); else the partials, slab z at out + z * slab_stride, ldo == nrows
  int64_t ldo, slab_stride;
};
// false: no such kernel (the caller reports it: there is no fallback). `stream` is a hipStream_t.
bool kernel_cross_launch(int dtype_is_f64, int profile, const KernelSchedule &S, const KernelCrossArgs &a, void *stream);
// Y[i + c ldy] = sum_z part[z * slab_stride + i + c nrows], z ascending
void kernel_cross_sum_launch(int dtype_is_f64, int64_t nrows, int b, int nslabs, const void *part, int64_t slab_stride, void *Y, int64_t ldy, void *stream);

#if defined(__HIPCC__) && defined(SLQ_KERNELCROSS_DEVICE)
// ---- device -------------------------------------------------------------------------------------------------------------
// Y = s phi(r2) W for column-major W (nsum x b, ldw) and Y (nrows x b, ldo). Two point sets: no diagonal rule, no sigma2 term.
// Element e of the 16 x NC tile of W -> (row, column): W is column-major, so a thread run should stay in one column; the LDS store
// wants a wave's 64 elements on distinct banks. fp32 (row stride NC + 4 words): 16 rows x 4 columns per wave do both. fp64 (row
// stride = 32 words mod 64): that shape would put 8 rows on one bank; 4 rows x 16 columns per wave - 32-byte runs of a column - is two
// lanes per bank, what a 512-byte store costs anyway.
struct KernelColumnLayout {
  static constexpr bool kDiagonal = false, kNoise = false, kScaled = false;  // (a cross product is defined on K0's points and profile: it ignores a diagonal scale)
  int64_t ldw, ldo;
  template <int NC> __device__ __forceinline__ static constexpr int chunk_cols() { return 16 * kKernelMaxColBlocks; }
  template <typename F, int NC> __device__ __forceinline__ static int w_row(int e) { return sizeof(F) == 8 ? ((e & 3) | ((e >> 4) & 12)) : (e & 15); }
  template <typename F, int NC> __device__ __forceinline__ static int w_col(int e) { return sizeof(F) == 8 ? (((e >> 2) & 15) | ((e >> 8) << 4)) : (e >> 4); }
  __device__ __forceinline__ int64_t w_off(int j, int g) const { return (int64_t)g * ldw + j; }
  __device__ __forceinline__ int64_t out_off(int i, int g) const { return (int64_t)g * ldo + i; }
  template <typename F> __device__ __forceinline__ F finish(F, const F *, int64_t, F v) const { return v; }
};
// (a kernel of its own name per layout: kernel_product of slq_kerneltile.hpp is the body)
template <typename F, int PROFILE, int NCB, int DQ>
__global__ __launch_bounds__(64 * kKernelWaves) void k_kernel_cross(int nrows, int rpad, int nsum, int spad, int dq, const F *__restrict__ rzt,
                                                                    const F *__restrict__ rnrm, const F *__restrict__ szt, const F *__restrict__ snrm,
                                                                    const F *__restrict__ params, const F *__restrict__ W, int64_t ldw, int b,
                                                                    int tiles_per_slab, F *__restrict__ out, int64_t ldo, int64_t slab_stride) {
  kernel_product<F, PROFILE, NCB, DQ>(nrows, rpad, nsum, spad, dq, rzt, rnrm, szt, snrm, params, W, b, tiles_per_slab, out, slab_stride, KernelColumnLayout{ldw, ldo});
}

// Y[i + c ldy] = the nslabs partials of element (i, c), added in slab order
template <typename F>
__global__ __launch_bounds__(256) void k_kernel_cross_sum(int64_t nrows, int b, int nslabs, const F *__restrict__ part, int64_t slab_stride, F *__restrict__ Y,
                                                          int64_t ldy) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= nrows * b) return;
  const int64_t c = e / nrows, i = e - c * nrows;
  const F *p = part + e;  // (a partial is nrows x b with leading dimension nrows)
  F v = p[0];
  for (int z = 1; z < nslabs; ++z) v += p[(int64_t)z * slab_stride];
  Y[(int64_t)c * ldy + i] = v;
}

template <typename F> static inline bool kernel_cross_launch_profile(int profile, const KernelSchedule &S, const KernelCrossArgs &a, hipStream_t st) {
  const dim3 g(S.nrow_blocks, S.ncol_chunks, S.nslabs), blk(64 * kKernelWaves);
  return kernel_for_profile(profile, [&](auto P) {
    return kernel_for_ncb(S.col_blocks, [&](auto NCB) {
      return kernel_for_dq(a.dq, [&](auto DQ) {
        k_kernel_cross<F, P(), NCB(), DQ()><<<g, blk, 0, st>>>(a.nrows, a.rpad, a.nsum, a.spad, a.dq, (const F *)a.rzt, (const F *)a.rnrm, (const F *)a.szt,
                                                             (const F *)a.snrm, (const F *)a.params, (const F *)a.W, a.ldw, a.b, S.tiles_per_slab, (F *)a.out,
                                                             a.ldo, a.slab_stride);
        return true;
      });
    });
  });
}
#endif  // __HIPCC__ && SLQ_KERNELCROSS_DEVICE

}  // namespace slq
