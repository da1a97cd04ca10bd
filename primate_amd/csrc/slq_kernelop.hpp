// slq_kernelop.hpp — the matrix-free kernel operator (slq_kernel_*): for n points in d dimensions
//   z_i = (x_i - mean(x)) / l   (rounded to the operator's dtype: the operator is DEFINED on these z)
//   r2_ij = max(0, |z_i|^2 + |z_j|^2 - 2 z_i.z_j), r2_ii = 0      A = s phi(r2) + sigma2 I
// with phi one of rbf, matern12, matern32, matern52. The product Y = A W never holds A: a 16 x 16 tile of z z^T is a small
// MFMA GEMM of the coordinates, goes through phi on the VALU and feeds, from the registers it was computed in, the MFMA GEMM
// with the probe panel. Operator memory is O(n d).
// Two parts:
//   host (plain C++, no HIP include; scripts/kernelop_check.cpp runs it under the host sanitizers)
//     kernel_validate   the arguments of slq_kernel_create / _set_parameters, naming the first bad value
//     kernel_column_means   the centre of the points: per dimension, the sum in row order in double, divided by n
//     kernel_schedule   row blocks, column chunks and j slabs of one product for (n, PW, NP, num_cus) (slq_debug_kernel_schedule)
//   device (hipcc only)
//     k_kernel_rescale  z and |z|^2 from the raw points, s and sigma2 into their device words
//     k_kernel_panel    T = A W for the panel layout of DESIGN.md §3
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdio>

namespace slq {

constexpr int kKernelMaxDim = 64;        // d <= 64: the z fragments of a wave's rows live in registers
constexpr int kKernelWaves = 8;          // waves per workgroup of k_kernel_panel
constexpr int kKernelRows = 16 * kKernelWaves;  // output rows per workgroup: 16 per wave
constexpr int kKernelMaxColBlocks = 16;  // 16-column accumulator tiles per wave: 256 columns, 64 fp64 accumulators per lane
constexpr int kKernelMaxSlabs = 16;      // j slabs (partial products summed in slab order by k_3term_slabs)

enum { KERNEL_RBF = 0, KERNEL_MATERN12 = 1, KERNEL_MATERN32 = 2, KERNEL_MATERN52 = 3, kNumKernelProfiles = 4 };
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
       KERNEL_BAD_OUTPUTSCALE, KERNEL_BAD_NOISE, KERNEL_BAD_POINT };
struct KernelBad {
  int what = KERNEL_OK;
  int64_t row = -1;  // KERNEL_BAD_POINT: the point; KERNEL_BAD_LENGTHSCALE: the dimension
  int64_t col = -1;  // KERNEL_BAD_POINT: the coordinate
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
  for (int64_t i = 0; i < n; ++i)
    for (int k = 0; k < d; ++k)
      if (!std::isfinite((double)pts[i * ldp + k])) { b.what = KERNEL_BAD_POINT, b.row = i, b.col = k, b.value = (double)pts[i * ldp + k]; return b; }
  return b;
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
// A workgroup owns kKernelRows output rows and 16 * col_blocks of the NP * PW panel columns (all of them up to 256: the K tile is
// evaluated once for both panels of a 256-probe fp64 plan) and walks j in tiles of 16. Small n: n / 128 workgroups do not fill
// the chip, so j is also cut into `nslabs` runs of whole tiles; slab z covers rows [slab_begin[z], slab_begin[z + 1]) and
// lands in its own raw panel; the slabs are summed in slab order (no atomics). nslabs minimises rounds of workgroups times
// the work of one, plus a small cost per slab - the rule of the dense operator's K split.
struct KernelSchedule {
  int rows_per_block = kKernelRows;
  int nrow_blocks = 0;
  int col_blocks = 0;   // 16-column tiles per workgroup: 1, 2, 4, 8 or 16
  int ncol_chunks = 0;  // workgroups along the columns (gridDim.y)
  int nslabs = 0;       // gridDim.z
  int tiles_per_slab = 0;
  int64_t slab_begin[kKernelMaxSlabs + 1] = {};
};
inline KernelSchedule kernel_schedule(int64_t n, int PW, int NP, int num_cus) {
  KernelSchedule S;
  const int64_t ncols = (int64_t)PW * NP;
  S.nrow_blocks = (int)((n + kKernelRows - 1) / kKernelRows);
  const int want = (int)((std::min<int64_t>(ncols, 16 * kKernelMaxColBlocks) + 15) / 16);
  S.col_blocks = 1;
  while (S.col_blocks < want) S.col_blocks *= 2;
  S.ncol_chunks = (int)((ncols + 16 * S.col_blocks - 1) / (16 * S.col_blocks));
  const int64_t ntiles = (n + 15) / 16;
  const double wgs = (double)S.nrow_blocks * S.ncol_chunks;
  double best = 1e300;
  int ks_best = 1;
  for (int ks = 1; ks <= kKernelMaxSlabs && ks <= ntiles; ++ks) {
    const double cost = std::ceil(wgs * ks / std::max(num_cus, 1)) / ks + 0.005 * ks;
    if (cost < best - 1e-12) best = cost, ks_best = ks;
  }
  S.tiles_per_slab = (int)((ntiles + ks_best - 1) / ks_best);
  S.nslabs = (int)((ntiles + S.tiles_per_slab - 1) / S.tiles_per_slab);  // (no empty slab)
  for (int z = 0; z <= S.nslabs; ++z) S.slab_begin[z] = std::min<int64_t>(n, (int64_t)z * S.tiles_per_slab * 16);
  S.slab_begin[S.nslabs] = n;
  return S;
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

typedef double kd4_t __attribute__((ext_vector_type(4)));
typedef float kf4_t __attribute__((ext_vector_type(4)));
template <typename F> struct KernelAcc;
template <> struct KernelAcc<double> { using type = kd4_t; };
template <> struct KernelAcc<float> { using type = kf4_t; };
__device__ __forceinline__ kd4_t kernel_mfma(double a, double b, kd4_t c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
__device__ __forceinline__ kf4_t kernel_mfma(float a, float b, kf4_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

template <typename F, int PROFILE> __device__ __forceinline__ F kernel_profile(F r2) {
#ifdef SLQ_KERNEL_PHI_ONE  // a measurement build (scripts/bench_kernelop.py): phi == 1, what the product costs without the profile
  return r2 < (F)0 ? r2 : (F)1;
#endif
  if constexpr (PROFILE == KERNEL_RBF) {
    return exp((F)-0.5 * r2);
  } else if constexpr (PROFILE == KERNEL_MATERN12) {
    return exp(-sqrt(r2));
  } else if constexpr (PROFILE == KERNEL_MATERN32) {
    const F a = (F)1.7320508075688772935 * sqrt(r2);
    return ((F)1 + a) * exp(-a);
  } else {
    const F a = (F)2.2360679774997896964 * sqrt(r2);
    return fma((F)(5.0 / 3.0), r2, (F)1 + a) * exp(-a);
  }
}

// T = A W. Grid (row blocks, column chunks, j slabs); a wave owns 16 rows I and NCB 16-column tiles of the panel columns
// [col0, col0 + 16 NCB) (column g of the plan is column g % PW of panel g / PW). Per tile J of 16 points:
//   G^T = z_J z_I^T   DQ MFMAs at most (d padded to 4 dq): A operand z_J from LDS (k-major: 16 consecutive words per k), B
//                     operand z_I from registers (loaded once). The result layout puts K^T[j][i = lane & 15] in the lane that
//                     must supply K[i = lane & 15][j] as the A operand of the second product: no shuffle, no LDS round trip;
//   K = phi(r2)       4 values per lane, once per (i, j), whatever NCB is;
//   acc += K W_J      4 NCB MFMAs, W_J (16 x 16 NCB) from LDS, staged once per workgroup.
// The next tile's W, z and norms are in flight in registers while this tile computes. Fragment layouts (cdna_hip_programming.md
// §3): A[m = l & 15][k = l >> 4], B[k = l >> 4][n = l & 15]; C rows (l >> 4) + 4 reg in fp64, 4 (l >> 4) + reg in fp32.
// s and sigma2 come from params (device memory: a captured graph sees a hyperparameter change). gridDim.z > 1: slab z of the
// raw partial products at out + z * slab_stride (sigma2 W in slab 0), summed in slab order by k_3term_slabs.
template <typename F, int PROFILE, int NCB, int DQ>
__global__ __launch_bounds__(64 * kKernelWaves) void k_kernel_panel(int n, int npad, int dq, const F *__restrict__ zt, const F *__restrict__ nrm,
                                                                    const F *__restrict__ params, const F *__restrict__ W, int log2pw, int ncols,
                                                                    F *__restrict__ out, int64_t slab_stride) {
  using V4 = typename KernelAcc<F>::type;
  constexpr bool F64 = sizeof(F) == 8;
  constexpr int NC = 16 * NCB;
  constexpr int WS = NC + (F64 ? (NC % 32 == 16 ? 0 : 16) : 4);  // row stride of the W tile: the 4 rows a read touches on distinct banks
  constexpr int NT = 64 * kKernelWaves;
  constexpr int WPT = (16 * NC + NT - 1) / NT;  // W elements per thread and tile
  constexpr int ZPT = (DQ * 4 * 16 + NT - 1) / NT;
  __shared__ __attribute__((aligned(16))) F Ws[16][WS];
  __shared__ __attribute__((aligned(16))) F Zs[DQ * 4][16];
  __shared__ F Ns[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int PW = 1 << log2pw;
  const int col0 = blockIdx.y * NC;
  const int i0 = blockIdx.x * kKernelRows + wave * 16;
  const int ntiles = npad >> 4;
  const int per = (ntiles + (int)gridDim.z - 1) / (int)gridDim.z;
  const int t_begin = min(ntiles, (int)blockIdx.z * per), t_end = min(ntiles, t_begin + per);

  // this wave's rows: z_I^T as the B operand of the first product, |z_i|^2 for the lane's column i = lr
  F zi[DQ];
  const bool i_ok = i0 + lr < npad;
#pragma unroll
  for (int q = 0; q < DQ; ++q) zi[q] = (q < dq && i_ok) ? zt[(int64_t)(4 * q + lk) * npad + i0 + lr] : (F)0;
  const F ni = i_ok ? nrm[i0 + lr] : (F)0;
  V4 acc[NCB];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) acc[cb] = (V4)(F)0;

  F wreg[WPT], zreg[ZPT], nreg = (F)0;
  auto fetch = [&](int t) {
    const int j0 = t * 16;
#pragma unroll
    for (int u = 0; u < WPT; ++u) {
      const int e = tid + u * NT, jj = e / NC, c = e % NC;
      const int j = j0 + jj, g = col0 + c;
      F v = (F)0;
      if (e < 16 * NC && j < n && g < ncols) v = W[((int64_t)(g >> log2pw) * n + j) * PW + (g & (PW - 1))];
      wreg[u] = v;
    }
#pragma unroll
    for (int u = 0; u < ZPT; ++u) {
      const int e = tid + u * NT, k = e >> 4, jj = e & 15;
      zreg[u] = (e < DQ * 64 && k < 4 * dq) ? zt[(int64_t)k * npad + j0 + jj] : (F)0;
    }
    if (tid < 16) nreg = nrm[j0 + tid];
  };
  auto stash = [&]() {
#pragma unroll
    for (int u = 0; u < WPT; ++u) {
      const int e = tid + u * NT;
      if (e < 16 * NC) Ws[e / NC][e % NC] = wreg[u];
    }
#pragma unroll
    for (int u = 0; u < ZPT; ++u) {
      const int e = tid + u * NT;
      if (e < DQ * 64) Zs[e >> 4][e & 15] = zreg[u];
    }
    if (tid < 16) Ns[tid] = nreg;
  };
  if (t_begin < t_end) {
    fetch(t_begin);
    stash();
  }
  __syncthreads();
  for (int t = t_begin; t < t_end; ++t) {
    const bool more = t + 1 < t_end;  // (uniform over the workgroup)
    if (more) fetch(t + 1);
    V4 g = (V4)(F)0;
#pragma unroll
    for (int q = 0; q < DQ; ++q)
      if (q < dq) g = kernel_mfma(Zs[4 * q + lk][lr], zi[q], g);
    F kv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int jr = F64 ? lk + 4 * r : 4 * lk + r;
      F r2 = fma((F)-2, g[r], ni + Ns[jr]);
      r2 = fmax(r2, (F)0);
      if (t * 16 + jr == i0 + lr) r2 = (F)0;
      kv[r] = kernel_profile<F, PROFILE>(r2);
    }
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int jr = F64 ? lk + 4 * r : 4 * lk + r;
        acc[cb] = kernel_mfma(kv[r], Ws[jr][cb * 16 + lr], acc[cb]);
      }
    __syncthreads();
    if (more) stash();
    __syncthreads();
  }
  const F s = params[0], sig = blockIdx.z == 0 ? params[1] : (F)0;
  F *o = out + (int64_t)blockIdx.z * slab_stride;
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) {
    const int g = col0 + cb * 16 + lr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + (F64 ? lk + 4 * r : 4 * lk + r);
      if (i < n && g < ncols) {
        const int64_t off = ((int64_t)(g >> log2pw) * n + i) * PW + (g & (PW - 1));
        o[off] = fma(sig, W[off], s * acc[cb][r]);
      }
    }
  }
}

// the launch for (dtype, profile, schedule, d): every instantiation is named here
struct KernelPanelArgs {
  int n, npad, dq;
  const void *zt, *nrm, *params, *W;
  int log2pw, ncols;
  void *out;
  int64_t slab_stride;
};
template <typename F, int PROFILE, int NCB> static inline void kernel_panel_launch_dq(const KernelSchedule &S, const KernelPanelArgs &a, hipStream_t st) {
  const dim3 g(S.nrow_blocks, S.ncol_chunks, S.nslabs), b(64 * kKernelWaves);
  if (a.dq <= 4)
    k_kernel_panel<F, PROFILE, NCB, 4><<<g, b, 0, st>>>(a.n, a.npad, a.dq, (const F *)a.zt, (const F *)a.nrm, (const F *)a.params, (const F *)a.W, a.log2pw, a.ncols, (F *)a.out, a.slab_stride);
  else
    k_kernel_panel<F, PROFILE, NCB, 16><<<g, b, 0, st>>>(a.n, a.npad, a.dq, (const F *)a.zt, (const F *)a.nrm, (const F *)a.params, (const F *)a.W, a.log2pw, a.ncols, (F *)a.out, a.slab_stride);
}
template <typename F, int PROFILE> static inline bool kernel_panel_launch_ncb(const KernelSchedule &S, const KernelPanelArgs &a, hipStream_t st) {
  switch (S.col_blocks) {
    case 1: kernel_panel_launch_dq<F, PROFILE, 1>(S, a, st); return true;
    case 2: kernel_panel_launch_dq<F, PROFILE, 2>(S, a, st); return true;
    case 4: kernel_panel_launch_dq<F, PROFILE, 4>(S, a, st); return true;
    case 8: kernel_panel_launch_dq<F, PROFILE, 8>(S, a, st); return true;
    case 16: kernel_panel_launch_dq<F, PROFILE, 16>(S, a, st); return true;
    default: return false;
  }
}
// false: no such kernel (the caller reports it: there is no fallback)
template <typename F> static inline bool kernel_panel_launch(int profile, const KernelSchedule &S, const KernelPanelArgs &a, hipStream_t st) {
  switch (profile) {
    case KERNEL_RBF: return kernel_panel_launch_ncb<F, KERNEL_RBF>(S, a, st);
    case KERNEL_MATERN12: return kernel_panel_launch_ncb<F, KERNEL_MATERN12>(S, a, st);
    case KERNEL_MATERN32: return kernel_panel_launch_ncb<F, KERNEL_MATERN32>(S, a, st);
    case KERNEL_MATERN52: return kernel_panel_launch_ncb<F, KERNEL_MATERN52>(S, a, st);
    default: return false;
  }
}
#endif  // __HIPCC__

}  // namespace slq
