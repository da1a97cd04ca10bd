// slq_kernelop.hpp — the matrix-free kernel operator (slq_kernel_*): for n points in d dimensions
//   z_i = (x_i - mean(x)) / l   (rounded to the operator's dtype: the operator is DEFINED on these z)
//   r2_ij = max(0, |z_i|^2 + |z_j|^2 - 2 z_i.z_j), r2_ii = 0      A = s phi(r2) + sigma2 I
// with phi one of rbf, matern12, matern32, matern52. The product Y = A W never holds A: a 16 x 16 tile of z z^T is a small
// MFMA GEMM of the coordinates, goes through phi on the VALU and feeds, from the registers it was computed in, the MFMA GEMM
// with the probe panel. Operator memory is O(n d). The tile walk, the profiles and the slab rule are those of slq_kerneltile.hpp;
// here is what is the operator's own:
//   host (plain C++, no HIP include; scripts/kernelop_check.cpp runs it under the host sanitizers)
//     kernel_validate   the arguments of slq_kernel_create / _set_parameters, naming the first bad value
//     kernel_validate_diag_scale   the diagonal scale c of slq_kernel_set_diag_scale, naming the first bad entry
//     kernel_column_means   the centre of the points: per dimension, the sum in row order in double, divided by n
//     kernel_schedule   row blocks, column chunks and j slabs of one product for (n, PW, NP, num_cus) (slq_debug_kernel_schedule)
//   device (hipcc only)
//     k_kernel_rescale  z and |z|^2 from the raw points, s and sigma2 into their device words
//     k_kernel_panel    T = A W for the panel layout of DESIGN.md §3: kernel_product on KernelPanelLayout
//     k_kernel_diag_scale   the diagonal scale rounded to the operator's dtype, zeros in the padding
//     k_kernel_panel_scaled T = (s diag(c) phi(r2) diag(c) + sigma2 I) W: kernel_product on KernelScaledPanelLayout
#pragma once

#include <cstdio>
#include <limits>

#include "slq_kerneltile.hpp"

namespace slq {

inline const char *kernel_profile_name(int id) {
  switch (id) {
    case KERNEL_RBF: return "rbf";
    case KERNEL_MATERN12: return "matern12";
    case KERNEL_MATERN32: return "matern32";
    case KERNEL_MATERN52: return "matern52";
    default: return "?";
  }
}

inline int kernel_dpad(int d) { return (d + 3) / 4 * 4; }
inline int64_t kernel_npad(int64_t n) { return (n + 15) / 16 * 16; }

// ---- validation -------------------------------------------------------------------------------------------------------
// what: the first argument that is not acceptable, in the order the entries document (0: all fine)
enum { KERNEL_OK = 0, KERNEL_BAD_N, KERNEL_BAD_DIM, KERNEL_BAD_LDP, KERNEL_BAD_PROFILE, KERNEL_BAD_NLS, KERNEL_BAD_LENGTHSCALE,
       KERNEL_BAD_OUTPUTSCALE, KERNEL_BAD_NOISE, KERNEL_BAD_POINT, KERNEL_BAD_SCALE_LENGTH, KERNEL_BAD_SCALE };
struct KernelBad {
  int what = KERNEL_OK;
  int64_t row = -1;  // KERNEL_BAD_POINT: the point; KERNEL_BAD_LENGTHSCALE: the dimension; KERNEL_BAD_SCALE: the entry; KERNEL_BAD_SCALE_LENGTH: the length given
  int64_t col = -1;  // KERNEL_BAD_POINT: the coordinate; KERNEL_BAD_SCALE_LENGTH: the operator's n
  double value = 0.0;
};

// the hyperparameters alone (slq_kernel_set_parameters): nls is 1 (a scalar broadcasts) or d
inline KernelBad kernel_validate_parameters(int d, const double *ls, int nls, double s, double noise) {
  KernelBad b;
  if (!ls || (nls != 1 && nls != d)) { b.what = KERNEL_BAD_NLS, b.row = nls; return b; }
  for (int k = 0; k < nls; ++k)
    if (!(ls[k] > 0.0) || !std::isfinite(ls[k])) { b.what = KERNEL_BAD_LENGTHSCALE, b.row = k, b.value = ls[k]; return b; }
  if (!(s > 0.0) || !std::isfinite(s)) { b.what = KERNEL_BAD_OUTPUTSCALE, b.value = s; return b; }
  if (!(noise >= 0.0) || !std::isfinite(noise)) { b.what = KERNEL_BAD_NOISE, b.value = noise; return b; }
  return b;
}

// the diagonal scale of slq_kernel_set_diag_scale: nc == n entries, each finite and >= 0 - also after its one rounding to the
// operator's dtype F (1e300 is finite, (float)1e300 is not: entries above F's largest number are refused). The first bad entry is named.
template <typename F> inline KernelBad kernel_validate_diag_scale(int64_t n, const double *c, int64_t nc) {
  KernelBad b;
  if (nc != n) { b.what = KERNEL_BAD_SCALE_LENGTH, b.row = nc, b.col = n; return b; }
  for (int64_t i = 0; i < n; ++i)
    if (!(c[i] >= 0.0) || !std::isfinite(c[i]) || c[i] > (double)std::numeric_limits<F>::max()) { b.what = KERNEL_BAD_SCALE, b.row = i, b.value = c[i]; return b; }
  return b;
}

// the first coordinate of n points (row-major, ldp words per point) that is not finite (what == KERNEL_OK: none)
template <typename F> inline KernelBad kernel_first_bad_point(int64_t n, int d, const F *pts, int64_t ldp) {
  KernelBad b;
  for (int64_t i = 0; i < n; ++i)
    for (int k = 0; k < d; ++k)
      if (!std::isfinite((double)pts[i * ldp + k])) { b.what = KERNEL_BAD_POINT, b.row = i, b.col = k, b.value = (double)pts[i * ldp + k]; return b; }
  return b;
}

// everything slq_kernel_create reads; pts == nullptr (points on the device): the points are not looked at
template <typename F>
inline KernelBad kernel_validate(int64_t n, int d, const F *pts, int64_t ldp, int profile, const double *ls, int nls, double s, double noise) {
  KernelBad b;
  if (n <= 0 || n >= ((int64_t)1 << 31) - 16) { b.what = KERNEL_BAD_N, b.row = n; return b; }
  if (d < 1 || d > kKernelMaxDim) { b.what = KERNEL_BAD_DIM, b.row = d; return b; }
  if (ldp < d) { b.what = KERNEL_BAD_LDP, b.row = ldp; return b; }
  if (profile < 0 || profile >= kNumKernelProfiles) { b.what = KERNEL_BAD_PROFILE, b.row = profile; return b; }
  b = kernel_validate_parameters(d, ls, nls, s, noise);
  if (b.what != KERNEL_OK || !pts) return b;
  return kernel_first_bad_point<F>(n, d, pts, ldp);
}

inline void kernel_bad_message(const KernelBad &b, char *buf, size_t len) {
  switch (b.what) {
    case KERNEL_BAD_N: snprintf(buf, len, "kernel operator: n = %lld points (1 <= n < 2^31 - 16)", (long long)b.row); break;
    case KERNEL_BAD_DIM: snprintf(buf, len, "kernel operator: d = %lld dimensions (1 <= d <= %d)", (long long)b.row, kKernelMaxDim); break;
    case KERNEL_BAD_LDP: snprintf(buf, len, "kernel operator: ldp = %lld is below d", (long long)b.row); break;
    case KERNEL_BAD_PROFILE: snprintf(buf, len, "kernel operator: unknown profile %lld (0 rbf, 1 matern12, 2 matern32, 3 matern52)", (long long)b.row); break;
    case KERNEL_BAD_NLS: snprintf(buf, len, "kernel operator: %lld lengthscales (1 or d, and not NULL)", (long long)b.row); break;
    case KERNEL_BAD_LENGTHSCALE: snprintf(buf, len, "kernel operator: lengthscale[%lld] = %g is not a positive finite number", (long long)b.row, b.value); break;
    case KERNEL_BAD_OUTPUTSCALE: snprintf(buf, len, "kernel operator: outputscale = %g is not a positive finite number", b.value); break;
    case KERNEL_BAD_NOISE: snprintf(buf, len, "kernel operator: noise = %g is not a finite number >= 0", b.value); break;
    case KERNEL_BAD_POINT: snprintf(buf, len, "kernel operator: point %lld, coordinate %lld is %g (points must be finite)", (long long)b.row, (long long)b.col, b.value); break;
    case KERNEL_BAD_SCALE_LENGTH: snprintf(buf, len, "kernel operator: the diagonal scale has %lld entries, the operator n = %lld points", (long long)b.row, (long long)b.col); break;
    case KERNEL_BAD_SCALE: snprintf(buf, len, "kernel operator: diag_scale[%lld] = %g is not a finite number >= 0 in the operator's dtype", (long long)b.row, b.value); break;
    default: snprintf(buf, len, "kernel operator: ok"); break;
  }
}

// The centre the points are shifted to: per dimension the sum over the points in row order, in double, divided by n (one
// defined order, so that a host model reproduces z bit for bit).
template <typename F> inline void kernel_column_means(int64_t n, int d, const F *pts, int64_t ldp, double *mean) {
  for (int k = 0; k < d; ++k) mean[k] = 0.0;
  for (int64_t i = 0; i < n; ++i)
    for (int k = 0; k < d; ++k) mean[k] += (double)pts[i * ldp + k];
  for (int k = 0; k < d; ++k) mean[k] /= (double)n;
}

// ---- the schedule of one product --------------------------------------------------------------------------------------
// kernel_product_schedule (slq_kerneltile.hpp) with the operator's points as row points and as summed points, the NP * PW panel
// columns as columns (column g of the plan is column g % PW of panel g / PW) and at most kKernelMaxSlabs slabs: the plan
// allocates 1 + slabs panels, slab z lands in its own raw panel and k_3term_slabs sums them in slab order.
inline KernelSchedule kernel_schedule(int64_t n, int PW, int NP, int num_cus) {
  return kernel_product_schedule(n, n, (int64_t)PW * NP, num_cus, kKernelMaxSlabs);
}

#ifdef __HIPCC__
// ---- device -------------------------------------------------------------------------------------------------------------
struct KernelScale {
  double mean[kKernelMaxDim];
  double ls[kKernelMaxDim];  // per dimension (a scalar already broadcast)
};

// z (transposed: zt[k][i], dpad x npad, zeros beyond d and n) and |z|^2 from the raw points (n x d, row-major); s and sigma2
// into params[0], params[1]. z = (F)(((double)x - mean) / l): one rounding to F after exact-order double arithmetic.
template <typename F>
__global__ __launch_bounds__(256) void k_kernel_rescale(int n, int npad, int d, int dpad, const F *__restrict__ raw, KernelScale sc, F *__restrict__ zt,
                                                        F *__restrict__ nrm, F *__restrict__ params, double s, double noise) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) params[0] = (F)s, params[1] = (F)noise;
  if (i >= npad) return;
  F acc = (F)0;
  for (int k = 0; k < dpad; ++k) {
    F z = (F)0;
    if (i < n && k < d) z = (F)(((double)raw[(int64_t)i * d + k] - sc.mean[k]) / sc.ls[k]);
    zt[(int64_t)k * npad + i] = z;
    acc = fma(z, z, acc);
  }
  nrm[i] = acc;
}

// T = A W for the panel layout of DESIGN.md §3: element (j, g) of W and of T at ((g / PW) n + j) PW + g % PW. Consecutive threads
// fetch consecutive columns of one row. One point set: the diagonal rule holds, and slab 0 adds sigma2 W.
struct KernelPanelLayout {
  static constexpr bool kDiagonal = true, kNoise = true, kScaled = false;
  int n, log2pw;
  template <int NC> __device__ __forceinline__ static constexpr int chunk_cols() { return NC; }
  template <typename F, int NC> __device__ __forceinline__ static int w_row(int e) { return e / NC; }
  template <typename F, int NC> __device__ __forceinline__ static int w_col(int e) { return e % NC; }
  __device__ __forceinline__ int64_t w_off(int j, int g) const { return ((int64_t)(g >> log2pw) * n + j) * (1 << log2pw) + (g & ((1 << log2pw) - 1)); }
  __device__ __forceinline__ int64_t out_off(int i, int g) const { return w_off(i, g); }
  template <typename F> __device__ __forceinline__ F finish(F sig, const F *W, int64_t off, F v) const { return fma(sig, W[off], v); }
};
// (a kernel of its own name per layout: kernel_product of slq_kerneltile.hpp is the body)
template <typename F, int PROFILE, int NCB, int DQ>
__global__ __launch_bounds__(64 * kKernelWaves) void k_kernel_panel(int n, int npad, int dq, const F *__restrict__ zt, const F *__restrict__ nrm,
                                                                    const F *__restrict__ params, const F *__restrict__ W, int log2pw, int ncols,
                                                                    int tiles_per_slab, F *__restrict__ out, int64_t slab_stride) {
  kernel_product<F, PROFILE, NCB, DQ>(n, npad, n, npad, dq, zt, nrm, zt, nrm, params, W, ncols, tiles_per_slab, out, slab_stride, KernelPanelLayout{n, log2pw});
}


// The diagonal scale as the product reads it: c rounded once to F, zeros in the padding [n, npad).
template <typename F> __global__ __launch_bounds__(256) void k_kernel_diag_scale(int n, int npad, const double *__restrict__ c64, F *__restrict__ c) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < npad) c[i] = i < n ? (F)c64[i] : (F)0;
}

// A = s diag(c) phi(r2) diag(c) + sigma2 I on the panel layout: KernelPanelLayout's addresses, bank pattern and
// epilogue (still one fma with sigma2 W), plus the npad words of c. c == 1 everywhere gives the bits of k_kernel_panel: the same
// summation order, and multiplying by 1 rounds nothing.
struct KernelScaledPanelLayout {
  static constexpr bool kDiagonal = true, kNoise = true, kScaled = true;
  int n, log2pw;
  const void *c;
  template <typename F> __device__ __forceinline__ const F *scale() const { return (const F *)c; }
  template <int NC> __device__ __forceinline__ static constexpr int chunk_cols() { return NC; }
  template <typename F, int NC> __device__ __forceinline__ static int w_row(int e) { return e / NC; }
  template <typename F, int NC> __device__ __forceinline__ static int w_col(int e) { return e % NC; }
  __device__ __forceinline__ int64_t w_off(int j, int g) const { return ((int64_t)(g >> log2pw) * n + j) * (1 << log2pw) + (g & ((1 << log2pw) - 1)); }
  __device__ __forceinline__ int64_t out_off(int i, int g) const { return w_off(i, g); }
  template <typename F> __device__ __forceinline__ F finish(F sig, const F *W, int64_t off, F v) const { return fma(sig, W[off], v); }
};
template <typename F, int PROFILE, int NCB, int DQ>
__global__ __launch_bounds__(64 * kKernelWaves) void k_kernel_panel_scaled(int n, int npad, int dq, const F *__restrict__ zt, const F *__restrict__ nrm,
                                                                           const F *__restrict__ params, const F *__restrict__ c, const F *__restrict__ W, int log2pw,
                                                                           int ncols, int tiles_per_slab, F *__restrict__ out, int64_t slab_stride) {
  kernel_product<F, PROFILE, NCB, DQ>(n, npad, n, npad, dq, zt, nrm, zt, nrm, params, W, ncols, tiles_per_slab, out, slab_stride, KernelScaledPanelLayout{n, log2pw, c});
}

struct KernelPanelArgs {
  int n, npad, dq;
  const void *zt, *nrm, *params, *W;
  int log2pw, ncols;
  void *out;
  int64_t slab_stride;
  const void *c = nullptr;  // the diagonal scale (npad words) of kernel_panel_scaled_launch; null: none
};
// false: no such kernel (the caller reports it: there is no fallback)
template <typename F> static inline bool kernel_panel_launch(int profile, const KernelSchedule &S, const KernelPanelArgs &a, hipStream_t st) {
  const dim3 g(S.nrow_blocks, S.ncol_chunks, S.nslabs), b(64 * kKernelWaves);
  return kernel_for_profile(profile, [&](auto P) {
    return kernel_for_ncb(S.col_blocks, [&](auto NCB) {
      return kernel_for_dq(a.dq, [&](auto DQ) {
        k_kernel_panel<F, P(), NCB(), DQ()><<<g, b, 0, st>>>(a.n, a.npad, a.dq, (const F *)a.zt, (const F *)a.nrm, (const F *)a.params, (const F *)a.W, a.log2pw,
                                                           a.ncols, S.tiles_per_slab, (F *)a.out, a.slab_stride);
        return true;
      });
    });
  });
}
// ... and the same ladder for an operator with a diagonal scale (a.c): k_kernel_panel_scaled
template <typename F> static inline bool kernel_panel_scaled_launch(int profile, const KernelSchedule &S, const KernelPanelArgs &a, hipStream_t st) {
  const dim3 g(S.nrow_blocks, S.ncol_chunks, S.nslabs), b(64 * kKernelWaves);
  return kernel_for_profile(profile, [&](auto P) {
    return kernel_for_ncb(S.col_blocks, [&](auto NCB) {
      return kernel_for_dq(a.dq, [&](auto DQ) {
        k_kernel_panel_scaled<F, P(), NCB(), DQ()><<<g, b, 0, st>>>(a.n, a.npad, a.dq, (const F *)a.zt, (const F *)a.nrm, (const F *)a.params, (const F *)a.c,
                                                                  (const F *)a.W, a.log2pw, a.ncols, S.tiles_per_slab, (F *)a.out, a.slab_stride);
        return true;
      });
    });
  });
}
#endif  // __HIPCC__

}  // namespace slq
