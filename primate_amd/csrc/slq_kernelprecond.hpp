// slq_kernelprecond.hpp — a pivoted-Cholesky preconditioner for the matrix-free kernel operator, fp64 only.
// K0 = s phi(r2) is the kernel matrix without noise, A = K0 + sigma2 I. L (n x r) is the greedy partial pivoted Cholesky factor of
// K0, P = L L^T + sigma2 I, and with the eigendecomposition L^T L = V diag(t) V^T
//   P^{-1/2} = M = sigma^-1 (I - L G L^T),  G = V diag(g(t)) V^T,  g(t) = (1 - (1 + t / sigma2)^{-1/2}) / t,
//   logdet P = sum log1p(t_i / sigma2) + n log sigma2.
// The preconditioned operator is B = M A M: logdet A = tr log B + logdet P and A^-1 y = M B^-1 M y, exactly, for any L.
// Two parts:
//   host (plain C++, no HIP include; scripts/kernelprecond_check.cpp runs it under the host sanitizers)
//     precond_rpad, precond_bpad  the padded rank (a multiple of 16) and the padded column count (a multiple of 64)
//     precond_apply_slabs         how the rows are cut into slabs for L^T W: a pure function of (n, columns, num_cus)
//     precond_scratch_words       what one apply needs behind it: the slab partials and G (L^T W)
//     precond_jacobi              cyclic Jacobi on the r x r Gram matrix, fixed sweep order
//     precond_g, precond_finish   g(t), G, H and logdet P from the eigendecomposition (H = (L^T L + sigma2 I)^-1: P^-1 = (I - L H L^T) / sigma2, §4.19)
//   device (hipcc only)
//     k_precond_init, k_precond_column   the factor: one launch per step, no host synchronisation in between
//     k_precond_lt, k_precond_gz, k_precond_nn   Zt = L^T W in row slabs, their sum in slab order times G, Y = c (X - L (G Zt))
//     k_precond_columns, k_precond_trace_add     columns of L or L H as a column-major matrix (operands of the gradient kernel), the
//                                                constant sigma^-2 tr D of tr(P^-1 D) (§4.19)
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "slq_kerneltile.hpp"  // kernel_profile, kernel_mfma, kd4_t

namespace slq {

constexpr int kPrecondMaxRank = 256;    // r <= 256: one thread of the reducer per factor column, 64 fragments of L per lane in k_precond_nn
constexpr int kPrecondMaxSlabs = 64;    // row slabs of L^T W (summed in slab order by k_precond_gz)
constexpr int kPrecondMaxParts = 1024;  // workgroups of a factor step: (max, index) partials the next step reduces
constexpr int kPrecondColsPerWg = 64;   // columns a workgroup of k_precond_lt owns: 16 per wave
constexpr int kPrecondThreads = 256;
constexpr int kPrecondChunkCols = 64;   // columns of L and L H one gradient update of the exact part takes (slq_kernel_precond_trace_grad)

inline int precond_rpad(int rank_max) { return (rank_max + 15) / 16 * 16; }
inline int64_t precond_bpad(int64_t cols) { return (cols + kPrecondColsPerWg - 1) / kPrecondColsPerWg * kPrecondColsPerWg; }
inline int precond_factor_parts(int64_t n) { return (int)std::min<int64_t>(kPrecondMaxParts, (n + kPrecondThreads - 1) / kPrecondThreads); }

// Zt = L^T W sums over the n rows: ceil(cols / 64) workgroups per slab do not fill the chip, so the rows are cut into nslabs runs
// of rows_per_slab (a multiple of 16; the last may be shorter), about four 4-wave workgroups per CU in all. The slab boundaries fix the
// summation order and therefore the bits: the rule reads nothing but its arguments.
struct PrecondSlabs {
  int nslabs = 1;
  int64_t rows_per_slab = 16;
};
inline PrecondSlabs precond_apply_slabs(int64_t n, int64_t cols, int num_cus) {
  const int64_t colwgs = std::max<int64_t>(1, (cols + kPrecondColsPerWg - 1) / kPrecondColsPerWg);
  const int64_t tiles = std::max<int64_t>(1, (n + 15) / 16);
  int64_t want = std::max<int64_t>(1, (4 * (int64_t)std::max(num_cus, 1) + colwgs - 1) / colwgs);
  want = std::min<int64_t>(std::min<int64_t>(want, kPrecondMaxSlabs), std::max<int64_t>(1, tiles / 4));  // (64 rows per slab at least)
  PrecondSlabs s;
  s.rows_per_slab = (tiles + want - 1) / want * 16;
  s.nslabs = (int)((n + s.rows_per_slab - 1) / s.rows_per_slab);  // (no empty slab)
  if (s.nslabs < 1) s.nslabs = 1;
  return s;
}
// doubles behind one apply on `cols` columns: [nslabs][bpad][rpad] partials, then [bpad][rpad] G (L^T W)
inline size_t precond_scratch_words(int64_t n, int64_t cols, int rpad, int num_cus) {
  const PrecondSlabs s = precond_apply_slabs(n, cols, num_cus);
  return (size_t)(s.nslabs + 1) * (size_t)precond_bpad(cols) * (size_t)rpad;
}
// ... and its bound over every column count a plan of that many columns may be asked for (the plan's region is sized before the slabs are known)
inline size_t precond_scratch_bound_words(int64_t cols, int rpad) { return (size_t)(kPrecondMaxSlabs + 1) * (size_t)precond_bpad(cols) * (size_t)rpad; }

// g(t) = (1 - (1 + x)^{-1/2}) / (x sigma2), x = t / sigma2: smooth at 0 (g(0) = 1 / (2 sigma2)), non-increasing, so the tiny and
// inaccurate eigenvalues of L^T L do no harm. Negative t (rounding of a zero eigenvalue) count as 0.
inline double precond_g(double t, double sigma2) {
  const double x = t > 0.0 ? t / sigma2 : 0.0;
  if (!(x > 0x1p-60)) return 0.5 / sigma2;  // (h = 1/2 - 3x/8 + ...: 1/2 to the last bit)
  const double h = -std::expm1(-0.5 * std::log1p(x)) / x;
  return std::min(h, 0.5) / sigma2;
}

// Cyclic Jacobi on the symmetric r x r matrix A (row-major, ld = r; destroyed: its diagonal ends as the eigenvalues), rows (p, q)
// in the fixed order p < q, row by row: A = V diag(t) V^T, V row-major with the eigenvectors as columns. A rotation is skipped
// where |a_pq| is negligible against sqrt(a_pp a_qq) or against the largest diagonal entry of the input (the Gram matrix of a
// factor with zero columns has exact zero rows). Returns the sweeps taken (kPrecondJacobiSweeps: not converged).
constexpr int kPrecondJacobiSweeps = 60;
inline int precond_jacobi(int r, double *A, double *V, double *t) {
  const double eps = std::numeric_limits<double>::epsilon();
  for (int i = 0; i < r; ++i)
    for (int j = 0; j < r; ++j) V[(size_t)i * r + j] = i == j ? 1.0 : 0.0;
  double dmax = 0.0;
  for (int i = 0; i < r; ++i) dmax = std::max(dmax, std::fabs(A[(size_t)i * r + i]));
  const double floor_abs = dmax * eps * 0x1p-10;
  int sweep = 0;
  for (; sweep < kPrecondJacobiSweeps; ++sweep) {
    int rotations = 0;
    for (int p = 0; p < r - 1; ++p)
      for (int q = p + 1; q < r; ++q) {
        const double apq = A[(size_t)p * r + q], app = A[(size_t)p * r + p], aqq = A[(size_t)q * r + q];
        const double mag = std::fabs(apq);
        if (mag <= floor_abs || mag <= 0.25 * eps * std::sqrt(std::fabs(app) * std::fabs(aqq))) continue;
        ++rotations;
        const double theta = (aqq - app) / (2.0 * apq);
        const double tn = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(tn * tn + 1.0), s = tn * c;
        for (int k = 0; k < r; ++k) {  // columns p, q
          const double akp = A[(size_t)k * r + p], akq = A[(size_t)k * r + q];
          A[(size_t)k * r + p] = c * akp - s * akq;
          A[(size_t)k * r + q] = s * akp + c * akq;
        }
        for (int k = 0; k < r; ++k) {  // rows p, q
          const double apk = A[(size_t)p * r + k], aqk = A[(size_t)q * r + k];
          A[(size_t)p * r + k] = c * apk - s * aqk;
          A[(size_t)q * r + k] = s * apk + c * aqk;
        }
        A[(size_t)p * r + q] = A[(size_t)q * r + p] = 0.0;
        for (int k = 0; k < r; ++k) {
          const double vkp = V[(size_t)k * r + p], vkq = V[(size_t)k * r + q];
          V[(size_t)k * r + p] = c * vkp - s * vkq;
          V[(size_t)k * r + q] = s * vkp + c * vkq;
        }
      }
    if (!rotations) break;
  }
  for (int i = 0; i < r; ++i) t[i] = A[(size_t)i * r + i];
  return sweep;
}

// h(t) = 1 / (t + sigma2): H = V diag(h(t)) V^T = (L^T L + sigma2 I)^-1. Negative t count as 0, as in g.
inline double precond_h(double t, double sigma2) { return 1.0 / ((t > 0.0 ? t : 0.0) + sigma2); }

// G = V diag(g(t)) V^T (r x r into an rpad x rpad row-major array, zeros in the padding), logdet P and the largest eigenvalue;
// H = V diag(h(t)) V^T in the same layout where H is not null (exactly symmetric: each pair is computed once)
struct PrecondSpectrum {
  double logdet_p = 0.0, t_max = 0.0;
};
inline PrecondSpectrum precond_finish(int64_t n, int r, int rpad, const double *V, const double *t, double sigma2, double *G, double *H = nullptr) {
  PrecondSpectrum sp;
  std::vector<double> gt((size_t)r), ht((size_t)r);
  for (int i = 0; i < r; ++i) {
    const double ti = std::max(t[i], 0.0);
    gt[(size_t)i] = precond_g(ti, sigma2);
    ht[(size_t)i] = precond_h(ti, sigma2);
    sp.logdet_p += std::log1p(ti / sigma2);
    sp.t_max = std::max(sp.t_max, ti);
  }
  sp.logdet_p += (double)n * std::log(sigma2);
  std::fill(G, G + (size_t)rpad * rpad, 0.0);
  for (int i = 0; i < r; ++i)
    for (int j = i; j < r; ++j) {
      double a = 0.0;
      for (int k = 0; k < r; ++k) a += V[(size_t)i * r + k] * gt[(size_t)k] * V[(size_t)j * r + k];
      G[(size_t)i * rpad + j] = G[(size_t)j * rpad + i] = a;
    }
  if (H) {
    std::fill(H, H + (size_t)rpad * rpad, 0.0);
    for (int i = 0; i < r; ++i)
      for (int j = i; j < r; ++j) {
        double a = 0.0;
        for (int k = 0; k < r; ++k) a += V[(size_t)i * r + k] * ht[(size_t)k] * V[(size_t)j * r + k];
        H[(size_t)i * rpad + j] = H[(size_t)j * rpad + i] = a;
      }
  }
  return sp;
}

#ifdef __HIPCC__
// ---- device -------------------------------------------------------------------------------------------------------------
// where element (row i, column g) of W, X and Y lives: a plan's panels (NP panels of n x PW, row-major), or columns ld apart
struct PrecondPanelLayout {
  int n, pw;
  __device__ __forceinline__ int64_t off(int i, int g) const { return ((int64_t)(g / pw) * n + i) * pw + g % pw; }
};
struct PrecondColumnLayout {
  int64_t ld;
  __device__ __forceinline__ int64_t off(int i, int g) const { return (int64_t)g * ld + i; }
};

// (value, index) with the larger value first, ties to the smaller index: the order of the pivot search
__device__ __forceinline__ void precond_take(double &v, int &i, double v2, int i2) {
  if (v2 > v || (v2 == v && i2 < i)) v = v2, i = i2;
}
// the best pair of the workgroup, in every thread (a tree over LDS: the same operands in the same order every time)
__device__ __forceinline__ void precond_wg_best(double &v, int &i, double *sv, int *si) {
  const int tid = threadIdx.x;
  sv[tid] = v, si[tid] = i;
  __syncthreads();
  for (int h = kPrecondThreads / 2; h > 0; h >>= 1) {
    if (tid < h) {
      double a = sv[tid];
      int ai = si[tid];
      precond_take(a, ai, sv[tid + h], si[tid + h]);
      sv[tid] = a, si[tid] = ai;
    }
    __syncthreads();
  }
  v = sv[0], i = si[0];
  __syncthreads();
}

// before step 0: the residual diagonal d = s, no pivots, rank 0, and the partials step 0 reduces: (s, 0) - the tie goes to row 0
__global__ __launch_bounds__(kPrecondThreads) void k_precond_init(int n, int rank_max, int nparts, const double *__restrict__ params, double *__restrict__ dres,
                                                                 int *__restrict__ pivots, int *__restrict__ rank, double *__restrict__ dpiv,
                                                                 double *__restrict__ pv, int *__restrict__ pi) {
  const int i = blockIdx.x * kPrecondThreads + threadIdx.x;
  const double s = params[0];
  if (i < n) dres[i] = s;
  if (i < rank_max) pivots[i] = -1, dpiv[i] = 0.0;
  if (i < nparts) pv[i] = i == 0 ? s : -1.0, pi[i] = 0;
  if (i == 0) *rank = 0;
}

// Step k of the factor. Every workgroup reduces the partials the previous launch left to the pivot p = argmax d (ties: the
// smallest index) - no atomics, no flags between workgroups: the kernel boundary is the synchronisation. Then, unless d_p is at
// or below thresh * s (the early stop: this and every later launch only hand their partials on), its rows i (grid-stride) get
//   L[i, k] = (K0[i, p] - L[i, :k] . L[p, :k]) / sqrt(d_p),  d_i <- max(0, d_i - L[i, k]^2),  d_p <- 0 exactly,
// rows with d_i == 0 already get L[i, k] = 0, and the workgroup leaves the (max, index) of its rows for step k + 1.
// K0[i, p] = s phi(r2), r2 = max(0, fma(-2, z_p . z_i, |z_p|^2 + |z_i|^2)), 0 exactly at i == p.
template <int PROFILE>
__global__ __launch_bounds__(kPrecondThreads) void k_precond_column(int n, int npad, int dim, const double *__restrict__ zt, const double *__restrict__ nrm,
                                                                   const double *__restrict__ params, double *__restrict__ L, int rpad, int k,
                                                                   double *__restrict__ dres, const double *__restrict__ pv_in, const int *__restrict__ pi_in,
                                                                   double *__restrict__ pv_out, int *__restrict__ pi_out, double thresh,
                                                                   int *__restrict__ pivots, int *__restrict__ rank, double *__restrict__ dpiv) {
  __shared__ double sv[kPrecondThreads];
  __shared__ int si[kPrecondThreads];
  __shared__ double Lp[kPrecondMaxRank];
  __shared__ double zp[kKernelMaxDim];
  const int tid = threadIdx.x, nparts = gridDim.x;
  double dp = -2.0;
  int p = 0x7fffffff;
  for (int w = tid; w < nparts; w += kPrecondThreads) precond_take(dp, p, pv_in[w], pi_in[w]);
  precond_wg_best(dp, p, sv, si);
  const double s = params[0];
  if (!(dp > thresh * s)) {  // (uniform over the grid: every workgroup reduced the same partials)
    if (tid == 0) pv_out[blockIdx.x] = pv_in[blockIdx.x], pi_out[blockIdx.x] = pi_in[blockIdx.x];
    return;
  }
  if (tid < k) Lp[tid] = L[(int64_t)p * rpad + tid];
  if (tid < dim) zp[tid] = zt[(int64_t)tid * npad + p];
  __syncthreads();
  const double np = nrm[p], root = sqrt(dp);
  double best = -1.0;
  int best_i = 0x7fffffff;
  for (int i = blockIdx.x * kPrecondThreads + tid; i < n; i += nparts * kPrecondThreads) {
    const double di = dres[i];
    double lik = 0.0;
    if (i == p || di != 0.0) {
      double g = 0.0;
      for (int c = 0; c < dim; ++c) g = fma(zp[c], zt[(int64_t)c * npad + i], g);
      double r2 = fmax(fma(-2.0, g, np + nrm[i]), 0.0);
      if (i == p) r2 = 0.0;
      double v = s * kernel_profile<double, PROFILE>(r2);
      const double *Li = L + (int64_t)i * rpad;
      for (int j = 0; j < k; ++j) v = fma(-Li[j], Lp[j], v);
      lik = v / root;
    }
    L[(int64_t)i * rpad + k] = lik;
    const double dn = i == p ? 0.0 : fmax(di - lik * lik, 0.0);
    dres[i] = dn;
    if (dn > best) best = dn, best_i = i;  // (i ascends: a tie keeps the smaller index)
  }
  precond_wg_best(best, best_i, sv, si);
  if (tid == 0) {
    pv_out[blockIdx.x] = best, pi_out[blockIdx.x] = best_i;
    if (blockIdx.x == 0) pivots[k] = p, dpiv[k] = dp, *rank = k + 1;
  }
}

// Zt = L^T W on the matrix cores, slab blockIdx.x of the rows into part[slab][g][m] (g the column, m the factor column). A
// workgroup of four waves owns 64 columns (blockIdx.y), a wave 16 of them and the MT row tiles of Zt from 16 MT blockIdx.z on: per 4
// rows one value of W and MT of L per lane, A[m = lane & 15][k = lane >> 4] = L[i0 + k][16 mt + m], B[k][n = lane & 15] =
// W[i0 + k][c0 + n]; the result's rows are (lane >> 4) + 4 reg. The loads of kPrecondLtDepth 4-row steps are issued before the first
// of their MFMAs: a wave alone on its SIMD otherwise waits out a memory round trip per step (measured: 160 us of a 240 us apply at
// n = 16384, r = 128, 128 columns). Columns at or beyond ncols enter as zeros and are stored (the partials hold bpad columns).
constexpr int kPrecondLtDepth = 4;
template <int MT, typename Layout>
__global__ __launch_bounds__(kPrecondThreads) void k_precond_lt(int n, const double *__restrict__ L, int rpad, const double *__restrict__ W, int ncols, Layout lay,
                                                               int rows_per_slab, double *__restrict__ part, int bpad) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lk = lane >> 4;
  const int nmt = rpad >> 4, mt0 = blockIdx.z * MT;
  const int g = (blockIdx.y * 4 + wave) * 16 + lr;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_slab;
  const int r1 = (int)std::min<int64_t>(n, r0 + rows_per_slab);
  kd4_t acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = (kd4_t)0.0;
  for (int i0 = (int)r0; i0 < r1; i0 += 4 * kPrecondLtDepth) {
    double bw[kPrecondLtDepth], av[kPrecondLtDepth][MT];
#pragma unroll
    for (int u = 0; u < kPrecondLtDepth; ++u) {
      const int i = i0 + 4 * u + lk;
      const bool ok = i < r1;
      bw[u] = (ok && g < ncols) ? W[lay.off(i, g)] : 0.0;
      const double *Li = L + (int64_t)i * rpad + 16 * mt0 + lr;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) av[u][mt] = (ok && mt0 + mt < nmt) ? Li[16 * mt] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kPrecondLtDepth; ++u)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[mt] = kernel_mfma(av[u][mt], bw[u], acc[mt]);
  }
  double *o = part + ((int64_t)blockIdx.x * bpad + g) * rpad;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
    if (mt0 + mt < nmt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) o[16 * (mt0 + mt) + lk + 4 * r] = acc[mt][r];
    }
}

// column g = blockIdx.x: t = the slab partials summed in slab order; out[g][m] = sum_j G[m][j] t[j] (G symmetric: read down
// its columns), or t itself where G is null (the Gram matrix L^T L of a factor)
__global__ __launch_bounds__(kPrecondThreads) void k_precond_gz(int rpad, int nslabs, const double *__restrict__ part, int bpad, const double *__restrict__ G,
                                                               double *__restrict__ out) {
  __shared__ double ts[kPrecondMaxRank];
  const int m = threadIdx.x, g = blockIdx.x;
  double t = 0.0;
  if (m < rpad)
    for (int z = 0; z < nslabs; ++z) t += part[((int64_t)z * bpad + g) * rpad + m];
  ts[m] = t;
  __syncthreads();
  if (m >= rpad) return;
  if (G) {
    t = 0.0;
    for (int j = 0; j < rpad; ++j) t = fma(G[(int64_t)j * rpad + m], ts[j], t);
  }
  out[(int64_t)g * rpad + m] = t;
}

// Y = c (X - L GZ), c = sigma^-1 from params[1], on the matrix cores. A wave owns 16 rows and keeps their rpad / 4 <= 4 MT
// fragments of L in registers (A[m = lane & 15][k = lane >> 4] = L[i0 + m][4 q + k]); per 16 columns the fragments of GZ
// (B[k][n = lane & 15] = GZ[c0 + n][4 q + k]) come from the cache. The column tiles are dealt over gridDim.y. X == Y is allowed:
// a lane reads an element before it writes it, and nobody else touches it.
template <int MT, typename Layout>
__global__ __launch_bounds__(kPrecondThreads) void k_precond_nn(int n, const double *__restrict__ L, int rpad, const double *__restrict__ GZ,
                                                               const double *__restrict__ params, const double *X, double *Y, int ncols, Layout lay) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lk = lane >> 4;
  const int nq = rpad >> 2;
  const int i0 = (blockIdx.x * 4 + wave) * 16;
  if (i0 >= n) return;
  double a[4 * MT];
  const bool row_ok = i0 + lr < n;
#pragma unroll
  for (int q = 0; q < 4 * MT; ++q) a[q] = (q < nq && row_ok) ? L[(int64_t)(i0 + lr) * rpad + 4 * q + lk] : 0.0;
  const double c = 1.0 / sqrt(params[1]);
  const int nct = (ncols + 15) >> 4;
  for (int ct = blockIdx.y; ct < nct; ct += gridDim.y) {
    const int g = ct * 16 + lr;
    const double *Z = GZ + (int64_t)g * rpad + lk;
    kd4_t acc = (kd4_t)0.0;
#pragma unroll
    for (int q = 0; q < 4 * MT; ++q)
      if (q < nq) acc = kernel_mfma(a[q], Z[4 * q], acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + lk + 4 * r;
      if (i < n && g < ncols) {
        const int64_t off = lay.off(i, g);
        Y[off] = c * (X[off] - acc[r]);
      }
    }
  }
}

// OUT[i, c] = sum_j L[i, j] Q[j, c0 + c] for c < nc <= 64 (the caller keeps c0 + nc <= rpad), OUT column-major with ld = n: nc
// columns of L Q as operand columns of the gradient kernel. Q (rpad x rpad, EXACTLY symmetric: H of precond_finish, read along its
// rows) goes through the matrix cores: a wave owns 16 rows and keeps their rpad / 4 <= 4 MT fragments of L in registers, as
// k_precond_nn does - here they are the B operand (B[k = lane >> 4][n = lane & 15] = L[i0 + n][4 q + k]) and Q's 16-column tile, from
// the cache, the A operand (A[m = lane & 15][k] = Q[c0 + 16 ct + m][4 q + k]), so that a lane's four results are four columns of ONE
// row and the 16 lanes of a group store 16 consecutive rows of a column. Q == NULL: the transposing copy OUT[i, c] = L[i, c0 + c],
// no MFMA. One writer per output word, no atomics, the sum over j in one fixed order: identical calls give identical bits. A
// slq_dmat has no padding rows (ld == n): nothing is written at or beyond row n.
template <int MT>
__global__ __launch_bounds__(kPrecondThreads) void k_precond_columns(int n, const double *__restrict__ L, int rpad, const double *__restrict__ Q, int c0, int nc,
                                                                    double *__restrict__ OUT) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lk = lane >> 4;
  const int i0 = (blockIdx.x * 4 + wave) * 16;
  if (i0 >= n) return;
  const int i = i0 + lr;
  const bool row_ok = i < n;
  const double *Li = L + (int64_t)(row_ok ? i : i0) * rpad;
  if (!Q) {
    for (int c = lk; c < nc; c += 4)
      if (row_ok) OUT[(int64_t)c * n + i] = Li[c0 + c];
    return;
  }
  const int nq = rpad >> 2;
  double b[4 * MT];
#pragma unroll
  for (int q = 0; q < 4 * MT; ++q) b[q] = (q < nq && row_ok) ? Li[4 * q + lk] : 0.0;
  for (int ct = 0; 16 * ct < nc; ++ct) {
    const int cq = 16 * ct + lr;  // the column of this lane's fragment of Q
    const double *Qc = Q + (int64_t)(c0 + (cq < nc ? cq : 0)) * rpad + lk;
    kd4_t acc = (kd4_t)0.0;
#pragma unroll
    for (int q = 0; q < 4 * MT; ++q)
      if (q < nq) acc = kernel_mfma(cq < nc ? Qc[4 * q] : 0.0, b[q], acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = 16 * ct + lk + 4 * r;
      if (row_ok && c < nc) OUT[(int64_t)c * n + i] = acc[r];
    }
  }
}

// vals[d] += a n / sigma2, vals[d + 1] += a n / sigma2: a sigma^-2 tr D of tr(P^-1 D) for the outputscale and the noise (tr D is n
// for both and 0 for every lengthscale), sigma2 read from the operator's device word. One thread.
__global__ void k_precond_trace_add(int d, double n, const double *__restrict__ params, double a, double *__restrict__ vals) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const double c = a * (n / params[1]);
    vals[d] += c;
    vals[d + 1] += c;
  }
}

// a run-time rpad to the instantiation compiled for it (MT = 1, 2, 4, 8, 16 tiles of 16 factor columns)
template <typename Fn> inline bool precond_for_mt(int rpad, Fn f) {
  const int nmt = rpad / 16;
  if (nmt <= 1) return f(std::integral_constant<int, 1>{});
  if (nmt <= 2) return f(std::integral_constant<int, 2>{});
  if (nmt <= 4) return f(std::integral_constant<int, 4>{});
  if (nmt <= 8) return f(std::integral_constant<int, 8>{});
  if (nmt <= 16) return f(std::integral_constant<int, 16>{});
  return false;
}

// OUT (n x nc, column-major, ld = n) = columns [c0, c0 + nc) of L (Q null) or of L Q; the caller has checked 0 <= c0, 1 <= nc <= 64, c0 + nc <= rpad
inline bool precond_columns_launch(int n, const double *L, int rpad, const double *Q, int c0, int nc, double *OUT, hipStream_t st) {
  return precond_for_mt(rpad, [&](auto MT) {
    k_precond_columns<MT()><<<dim3((n + 63) / 64), dim3(kPrecondThreads), 0, st>>>(n, L, rpad, Q, c0, nc, OUT);
    return true;
  });
}

// out[g][m] = (G or I) sum over the rows of L[i][m] W[i][g], g < bpad(ncols): the slab partials go to scratch, out may follow them
template <typename Layout>
inline bool precond_lt_launch(int n, const double *L, int rpad, const double *G, const double *W, int ncols, const Layout &lay, double *scratch, double *out, int num_cus,
                              hipStream_t st) {
  const PrecondSlabs S = precond_apply_slabs(n, ncols, num_cus);
  const int bpad = (int)precond_bpad(ncols);
  const int nmt = rpad / 16;
  if (nmt < 1 || nmt > kPrecondMaxRank / 16) return false;
  // (row tiles of Zt per wave: 4, 2 or 1, the rest of them along gridDim.z - more waves, each with fewer steps' worth of loads to wait for)
  const auto launch = [&](auto MT) {
    k_precond_lt<MT(), Layout><<<dim3(S.nslabs, bpad / kPrecondColsPerWg, (nmt + MT() - 1) / MT()), dim3(kPrecondThreads), 0, st>>>(n, L, rpad, W, ncols, lay,
                                                                                                                           (int)S.rows_per_slab, scratch, bpad);
  };
  if (nmt >= 4) launch(std::integral_constant<int, 4>{});
  else if (nmt >= 2) launch(std::integral_constant<int, 2>{});
  else launch(std::integral_constant<int, 1>{});
  k_precond_gz<<<dim3(bpad), dim3(kPrecondThreads), 0, st>>>(rpad, S.nslabs, scratch, bpad, G, out);
  return true;
}
// Y = M X for ncols columns in the layout `lay` (X == Y allowed); scratch: precond_scratch_words(n, ncols, rpad, num_cus) doubles
template <typename Layout>
inline bool precond_apply_launch(int n, const double *L, int rpad, const double *G, const double *params, const double *X, double *Y, int ncols, const Layout &lay,
                                 double *scratch, int num_cus, hipStream_t st) {
  const PrecondSlabs S = precond_apply_slabs(n, ncols, num_cus);
  const int bpad = (int)precond_bpad(ncols);
  double *gz = scratch + (size_t)S.nslabs * bpad * rpad;
  if (!precond_lt_launch(n, L, rpad, G, X, ncols, lay, scratch, gz, num_cus, st)) return false;
  const int rowwgs = (n + 63) / 64, nct = (ncols + 15) / 16;
  const int ywgs = std::max(1, std::min(nct, (2 * std::max(num_cus, 1) + rowwgs - 1) / rowwgs));
  return precond_for_mt(rpad, [&](auto MT) {
    k_precond_nn<MT(), Layout><<<dim3(rowwgs, ywgs), dim3(kPrecondThreads), 0, st>>>(n, L, rpad, gz, params, X, Y, ncols, lay);
    return true;
  });
}
// the rank_max steps of the factor, back to back on `st`. part: 2 x nparts doubles, then 2 x nparts ints (ping-pong partials)
inline bool precond_factor_launch(int profile, int n, int npad, int dim, const double *zt, const double *nrm, const double *params, double *L, int rpad, int rank_max,
                                  double thresh, double *dres, int *pivots, int *rank, double *dpiv, double *pv, int *pi, hipStream_t st) {
  const int nparts = precond_factor_parts(n);
  const int init_wgs = (std::max(std::max(n, rank_max), nparts) + kPrecondThreads - 1) / kPrecondThreads;
  k_precond_init<<<dim3(init_wgs), dim3(kPrecondThreads), 0, st>>>(n, rank_max, nparts, params, dres, pivots, rank, dpiv, pv, pi);
  return kernel_for_profile(profile, [&](auto P) {
    for (int k = 0; k < rank_max; ++k) {
      const int a = k & 1, b = a ^ 1;
      k_precond_column<P()><<<dim3(nparts), dim3(kPrecondThreads), 0, st>>>(n, npad, dim, zt, nrm, params, L, rpad, k, dres, pv + (size_t)a * nparts, pi + (size_t)a * nparts,
                                                                          pv + (size_t)b * nparts, pi + (size_t)b * nparts, thresh, pivots, rank, dpiv);
    }
    return true;
  });
}
#endif  // __HIPCC__

}  // namespace slq
