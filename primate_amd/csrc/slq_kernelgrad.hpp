// slq_kernelgrad.hpp — hyperparameter gradients of the matrix-free kernel operator (slq_kernel_grad_*). For the
// operator A = s phi(r2) + sigma2 I of slq_kernelop.hpp and two device matrices Z, W (n x m, fp64, column-major), with
//   C_ij = sum_c Z_ic W_jc,   D_ijk = z_ik - z_jk,   chi = -2 dphi/dr2
// one update computes the d + 2 sums
//   g_l[k]   = (s / l_k) sum_ij C_ij chi(r2_ij) D_ijk^2      = sum_c Z_c^T (dA/dl_k) W_c
//   g_s      =           sum_ij C_ij phi(r2_ij)              (dA/ds = phi)
//   g_sigma2 =           sum_i  C_ii                         (dA/dsigma2 = I)
// W = probes, Z = f'(A) probes: the Girard-Hutchinson estimate of d tr f(A) / d theta; Z = W = A^-1 y: the data-fit term. Neither A
// nor C is ever held: a 16 x 16 tile of each is one small MFMA GEMM, both land in the same lanes, and the sums are taken from there.
// The tile walk, r2, the profiles (phi with chi) and the slab rule are those of slq_kerneltile.hpp; here is what is the gradient's own:
//   host (plain C++, no HIP include; scripts/kernelgrad_check.cpp runs it under the host sanitizers)
//     kernel_grad_schedule   row blocks, j slabs and column chunks of one update for (n, m, num_cus) (slq_debug_kernel_grad_schedule)
//   device (hipcc only)
//     k_kernel_grad          one partial of dpad + 2 words per workgroup for one column chunk
//     k_kernel_grad_sum      the partials summed in workgroup order, scaled, folded into the accumulator's values
#pragma once

#include "slq_kernelop.hpp"

namespace slq {

constexpr int kKernelGradCols = 64;  // columns of Z and W one launch contracts: 16 fp64 B fragments of Z_I per lane

// ---- the schedule of one update -----------------------------------------------------------------------------------------
// Row blocks and j slabs by kernel_slab_split for one column chunk per workgroup - kernel_schedule's slabs of a 16-column product (a launch per chunk: the chunks of a
// wider m run one after the other on the stream and each folds into the values); slab z covers the points
// [slab_begin[z], slab_begin[z + 1]) - whole tiles of 16, tiles_per_slab of them but for the last.
struct KernelGradSchedule {
  int rows_per_block = kKernelRows;
  int nrow_blocks = 0;
  int chunk_cols = kKernelGradCols;
  int ncol_chunks = 0;  // launches of one update
  int nslabs = 0;       // gridDim.y
  int tiles_per_slab = 0;
  int64_t slab_begin[kKernelMaxSlabs + 1] = {};
  int64_t nparts() const { return (int64_t)nrow_blocks * nslabs; }  // workgroups, and partials, of one launch
};
inline KernelGradSchedule kernel_grad_schedule(int64_t n, int m, int num_cus) {
  KernelGradSchedule S;
  S.nrow_blocks = (int)((n + kKernelRows - 1) / kKernelRows);
  S.ncol_chunks = (m + kKernelGradCols - 1) / kKernelGradCols;
  const KernelSlabSplit s = kernel_slab_split((n + 15) / 16, (double)S.nrow_blocks, num_cus, kKernelMaxSlabs);  // (one column chunk per workgroup, whatever its width)
  S.nslabs = s.nslabs, S.tiles_per_slab = s.tiles_per_slab;
  kernel_slab_begin(s, n, S.slab_begin);
  return S;
}

#ifdef __HIPCC__
// ---- device -------------------------------------------------------------------------------------------------------------
struct KernelGradScale {
  double ls[kKernelMaxDim];  // the operator's host scale at update time, per dimension
};

// Grid (row blocks, j slabs); a wave owns 16 rows I and walks its slab's j in tiles of 16 (KernelTile, kernel_tile_walk). Per tile J:
//   G^T, r2           of KernelTile - the operator's operands in the operator's order, so r2 carries the operator's bits, with its
//                     clamp and its diagonal rule;
//   C^T = W_J Z_I^T   MQ MFMAs at most (the chunk's mc <= 64 columns padded to 4 mq): A operand W_J from LDS (column-major: 16
//                     consecutive words per column), B operand Z_I from registers (loaded once). C^T[j][i] lands in the lane that
//                     holds G^T[j][i]: lane (lr, lk) has i = lr and j = lk + 4 reg;
//   phi, chi          once per (i, j); as += phi c, ad += c on the diagonal, b = chi c;
//   per dimension     the four lanes (lr, 0..3) hold between them the 16 values b of row i = lr and, as their B fragments of the
//                     first product, the coordinates k = 4 q + lk of z_i. Each takes the other three lanes' b by shuffles and adds
//                     b (z_ik - z_jk)^2 over the 16 j for ITS k (z_jk from the LDS tile of the first product): differences, no
//                     cancellation, for every d <= 64, with dq accumulators per lane.
// Then lanes (the 16 lr of a k; all 64 for the two scalars), waves, and ONE partial of dpad + 2 words per workgroup at
// part[(blockIdx.y * gridDim.x + blockIdx.x) * (dpad + 2)]: k < dpad the raw sums per dimension, [dpad] sum C phi, [dpad + 1] sum C_ii
// (no atomics: the bits are the same run to run). A term passes through at most npad additions in its lane, 4 + 8 in the workgroup.
// Rows i >= n and points j >= n enter with Z = 0 and W = 0: c = 0, and phi, chi are finite at the zero padding of z.
template <int PROFILE, int DQ>
__global__ __launch_bounds__(64 * kKernelWaves) void k_kernel_grad(int n, int npad, int dq, const double *__restrict__ zt, const double *__restrict__ nrm,
                                                                   const double *__restrict__ Z, const double *__restrict__ W, int mc, int tiles_per_slab,
                                                                   double *__restrict__ part) {
  using T = KernelTile<double, DQ>;
  constexpr int MQ = kKernelGradCols / 4;
  constexpr int NT = T::NT;
  constexpr int WPT = (16 * kKernelGradCols + NT - 1) / NT;
  __shared__ __attribute__((aligned(16))) double Ws[kKernelGradCols][16];
  __shared__ __attribute__((aligned(16))) double Zs[DQ * 4][16];
  __shared__ double Ns[16];
  __shared__ double Red[kKernelWaves][DQ * 4 + 2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int i0 = blockIdx.x * kKernelRows + wave * 16;
  int t_begin, t_end;
  kernel_slab_tiles<int>(npad >> 4, tiles_per_slab, (int)blockIdx.y, &t_begin, &t_end);
  const int mq = (mc + 3) >> 2;

  // this wave's rows: z_I^T and Z_I^T as B operands, |z_i|^2 for the lane's column i = lr
  double zi[DQ], ni, zc[MQ];
  T::rows(zt, nrm, npad, dq, i0, lr, lk, zi, ni);
  const bool i_ok = i0 + lr < n;
#pragma unroll
  for (int q = 0; q < MQ; ++q) zc[q] = (i_ok && 4 * q + lk < mc) ? Z[(int64_t)(4 * q + lk) * n + i0 + lr] : 0.0;
  double acc[DQ], as = 0.0, ad = 0.0;
#pragma unroll
  for (int q = 0; q < DQ; ++q) acc[q] = 0.0;

  double wreg[WPT], zreg[T::ZPT], nreg = 0.0;
  auto fetch = [&](int t) {
    const int j0 = t * 16;
#pragma unroll
    for (int u = 0; u < WPT; ++u) {
      const int e = tid + u * NT, c = e >> 4, j = j0 + (e & 15);
      wreg[u] = (c < mc && j < n) ? W[(int64_t)c * n + j] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < T::ZPT; ++u) {
      const int e = tid + u * NT, k = e >> 4, jj = e & 15;
      zreg[u] = (e < DQ * 64 && k < 4 * dq) ? zt[(int64_t)k * npad + j0 + jj] : 0.0;
    }
    if (tid < 16) nreg = nrm[j0 + tid];
  };
  auto stash = [&]() {
#pragma unroll
    for (int u = 0; u < WPT; ++u) {
      const int e = tid + u * NT;
      if (e < 16 * kKernelGradCols) Ws[e >> 4][e & 15] = wreg[u];
    }
    T::stash(Zs, Ns, tid, zreg, nreg);
  };
  kernel_tile_walk(t_begin, t_end, fetch, stash, [&](int t) {
    const kd4_t g = T::gram(Zs, zi, dq, lr, lk);
    kd4_t c = (kd4_t)0.0;
#pragma unroll
    for (int q = 0; q < MQ; ++q)
      if (q < mq) c = kernel_mfma(Ws[4 * q + lk][lr], zc[q], c);
    double b[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool diag = t * 16 + T::jr(lk, r) == i0 + lr;
      double phi, chi;
      kernel_profile_pair<double, PROFILE>(T::r2(g, r, ni, Ns, lk, diag), phi, chi);
      as = fma(phi, c[r], as);
      if (diag) ad += c[r];
      b[r] = chi * c[r];
    }
#pragma unroll
    for (int src = 0; src < 4; ++src)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double bj = __shfl(b[r], lr + 16 * src, 64);  // chi c of the pair (i = lr, j = src + 4 r)
#pragma unroll
        for (int q = 0; q < DQ; ++q)
          if (q < dq) {
            const double dlt = zi[q] - Zs[4 * q + lk][src + 4 * r];
            acc[q] = fma(bj, dlt * dlt, acc[q]);
          }
      }
  });
  // lanes: the 16 lr of a coordinate; all 64 for the two scalars
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) {
#pragma unroll
    for (int q = 0; q < DQ; ++q) acc[q] += __shfl_xor(acc[q], off, 64);
  }
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) as += __shfl_xor(as, off, 64), ad += __shfl_xor(ad, off, 64);
  if (lr == 0) {
#pragma unroll
    for (int q = 0; q < DQ; ++q) Red[wave][4 * q + lk] = acc[q];
  }
  if (lane == 0) Red[wave][DQ * 4] = as, Red[wave][DQ * 4 + 1] = ad;
  __syncthreads();
  // waves, in wave order
  const int dpad = 4 * dq;
  if (tid < dpad + 2) {
    const int src = tid < dpad ? tid : DQ * 4 + (tid - dpad);
    double v = 0.0;
#pragma unroll
    for (int w = 0; w < kKernelWaves; ++w) v += Red[w][src];
    part[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (dpad + 2) + tid] = v;
  }
}

// vals[t] = beta vals[t] + alpha scale_t sum_p part[p][t], the nparts partials in workgroup order: scale s / l_t for t < d (s from
// the operator's device words), 1 for the outputscale [d] and the noise [d + 1]. beta == 0 does not read vals.
__global__ __launch_bounds__(128) void k_kernel_grad_sum(int d, int dpad, int64_t nparts, const double *__restrict__ part, const double *__restrict__ params,
                                                         KernelGradScale sc, double alpha, double beta, double *__restrict__ vals) {
  const int t = threadIdx.x;
  if (t >= d + 2) return;
  const int src = t < d ? t : dpad + (t - d);
  double v = 0.0;
  for (int64_t p = 0; p < nparts; ++p) v += part[p * (dpad + 2) + src];
  if (t < d) v *= params[0] / sc.ls[t];
  const double old = beta == 0.0 ? 0.0 : beta * vals[t];
  vals[t] = fma(alpha, v, old);
}

// false: no such kernel (the caller reports it: there is no fallback)
struct KernelGradArgs {
  int n, npad, dq;
  const double *zt, *nrm, *Z, *W;
  int mc, tiles_per_slab;
  double *part;
};
static inline bool kernel_grad_launch(int profile, const KernelGradSchedule &S, const KernelGradArgs &a, hipStream_t st) {
  const dim3 g(S.nrow_blocks, S.nslabs), b(64 * kKernelWaves);
  return kernel_for_profile(profile, [&](auto P) {
    return kernel_for_dq(a.dq, [&](auto DQ) {
      k_kernel_grad<P(), DQ()><<<g, b, 0, st>>>(a.n, a.npad, a.dq, a.zt, a.nrm, a.Z, a.W, a.mc, a.tiles_per_slab, a.part);
      return true;
    });
  });
}
#endif  // __HIPCC__

}  // namespace slq
