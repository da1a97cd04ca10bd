// slq_kernelpointgrad.hpp — gradients of the matrix-free kernel operator with respect to the POINTS (slq_kernel_pointgrad_*;
// DESIGN.md §4.20). For "row" points z_a (m of them), "summed" points z_j (n of them), a row-side factor U (m x b) and a summed-side
// factor W (n x b), both fp64 and column-major,
//   C_aj = sum_c U_ac W_jc,   chi = -2 dphi/dr2,   R[a][k] = -(s / l_k) sum_j C_aj chi(r2_aj) (z_ak - z_jk)        m x d
// is the gradient of sum_c U_c^T K(rows, summed) W_c in the row points (centring drops out of a difference: d/dx = (1 / l) d/dz).
//   cross form     rows = the new points z* of a slq_kernel_cross, summed = the training points, no diagonal rule: R(U, W)
//   training form  both sets the operator's points, its diagonal rule: P = R(Z, W) + R(W, Z) - two passes of the same kernel
// Neither A nor C nor dA/dx is held. The per-coordinate term is a DIFFERENCE of the two z, never rowsum(B) z_a - B z_J: coincident
// points contribute exactly 0 whatever chi is (matern12's chi grows like 1 / r). The tile walk, r2, the profiles and the slab rule are
// those of slq_kerneltile.hpp - r2 carries the operator's bits. Here is what is the point gradient's own:
//   host (plain C++, no HIP include; scripts/kernelpointgrad_check.cpp runs it under the host sanitizers)
//     kernel_pointgrad_schedule   row blocks and slabs of one pass for (nrows, nsum, num_cus) (slq_debug_kernel_pointgrad_schedule)
//   device (hipcc only)
//     k_kernel_pointgrad          one slab partial [slab][row][dpad] of the raw sums for one chunk of at most 64 factor columns
//     k_kernel_pointgrad_sum      the slab partials added in slab order, scaled by -s / l_k, folded into the accumulator's values
//   The instantiations of k_kernel_pointgrad (4 profiles x 2 coordinate depths) live in slq_kernelpointgrad.hip, a translation unit of
//   their own; slq.hip sees only kernel_pointgrad_launch / kernel_pointgrad_sum_launch.
#pragma once

#include "slq_kerneltile.hpp"

namespace slq {

constexpr int kKernelPointGradCols = 64;  // factor columns one launch contracts: 16 fp64 B fragments of U_I per lane

// ---- the schedule of one pass -------------------------------------------------------------------------------------------
// Row blocks of kKernelRows row points; the summed points cut into slabs by kernel_slab_split with the cross product's cap (a
// cross-form gradient at a few new points is one row block, as a forward cross product is). Slab z covers the points
// [slab_begin[z], slab_begin[z + 1]) - whole tiles of 16, tiles_per_slab of them but for the last - and lands in a partial of its
// own. The schedule does not depend on the number of factor columns: a wider factor is further launches with the same grid.
struct KernelPointGradSchedule {
  int rows_per_block = kKernelRows;
  int nrow_blocks = 0;   // gridDim.x
  int chunk_cols = kKernelPointGradCols;
  int nslabs = 0;        // gridDim.y
  int tiles_per_slab = 0;
  int64_t slab_begin[kKernelCrossMaxSlabs + 1] = {};
};
inline KernelPointGradSchedule kernel_pointgrad_schedule(int64_t nrows, int64_t nsum, int num_cus) {
  KernelPointGradSchedule S;
  S.nrow_blocks = (int)((nrows + kKernelRows - 1) / kKernelRows);
  const KernelSlabSplit s = kernel_slab_split((nsum + 15) / 16, (double)S.nrow_blocks, num_cus, kKernelCrossMaxSlabs);
  S.nslabs = s.nslabs, S.tiles_per_slab = s.tiles_per_slab;
  kernel_slab_begin(s, nsum, S.slab_begin);
  return S;
}

// the operator's host scale at update time, per dimension (as KernelGradScale of slq_kernelgrad.hpp)
struct KernelPointGradScale {
  double ls[kKernelMaxDim];
};

// what a pass reads and writes (plain pointers: the launch functions are defined in slq_kernelpointgrad.hip and called from slq.hip)
struct KernelPointGradArgs {
  int nrows, rpad;  // row points: count, count rounded up to 16
  int nsum, spad;   // summed points
  int dq;           // dpad / 4
  int diagonal;     // 1: both sets are the operator's points and r2 = 0 where the summed point IS the row point
  const double *rzt, *rnrm;  // row points: z transposed (dpad x rpad), |z|^2 (rpad)
  const double *szt, *snrm;  // summed points
  const double *U;           // nrows x mc, column-major with leading dimension nrows
  const double *W;           // nsum x mc, column-major with leading dimension nsum
  int mc;                    // 1 <= mc <= kKernelPointGradCols
  double *part;              // nslabs x nrows x dpad
};
// false: no such kernel (the caller reports it: there is no fallback). `stream` is a hipStream_t.
bool kernel_pointgrad_launch(int profile, const KernelPointGradSchedule &S, const KernelPointGradArgs &a, void *stream);
// vals[a * d + k] = beta vals[a * d + k] + alpha (-s / l_k) sum_z part[z][a][k], z ascending; s = params[0] on the device
void kernel_pointgrad_sum_launch(int64_t nrows, int d, int dpad, int nslabs, const double *part, const double *params, const KernelPointGradScale &sc,
                                 double alpha, double beta, double *vals, void *stream);

#if defined(__HIPCC__) && defined(SLQ_KERNELPOINTGRAD_DEVICE)
// ---- device -------------------------------------------------------------------------------------------------------------
// Grid (row blocks, slabs); a wave owns 16 rows I and walks its slab's j in tiles of 16 (KernelTile, kernel_tile_walk). Per tile J:
//   G^T, r2           of KernelTile - the operator's operands in the operator's order, its clamp and, where `diagonal`, its rule;
//   C^T = W_J U_I^T   MQ MFMAs at most (the chunk's mc <= 64 columns padded to 4 mq): A operand W_J from LDS (column-major: 16
//                     consecutive words per column), B operand U_I from registers (loaded once). C^T[j][i] lands in the lane that
//                     holds G^T[j][i]: lane (lr, lk) has i = lr and j = lk + 4 reg;
//   b = chi c         once per (i, j);
//   per coordinate    the four lanes (lr, 0..3) hold between them the 16 values b of row i = lr and, as their B fragments of the
//                     first product, the coordinates k = 4 q + lk of z_i. Each takes the other three lanes' b by shuffles and adds
//                     b (z_ik - z_jk) over the 16 j for ITS k (z_jk from the LDS tile of the first product): a difference, so a
//                     coincident pair adds b * 0 = 0 exactly; dq accumulators per lane.
// What k_kernel_grad does from here - square, reduce over the rows - is what this kernel does not: lane (lr, lk) ends with the sums
// of row i0 + lr for the coordinates 4 q + lk and writes them to part[(slab * nrows + row) * dpad + k]. No reduction across lanes
// or waves, no atomics: the bits are the same run to run. A term passes through at most spad additions here. Rows i >= nrows and
// points j >= nsum enter with U = 0 and W = 0: c = 0, and chi is finite at the zero padding of z. Rows i >= nrows are not stored.
template <int PROFILE, int DQ>
__global__ __launch_bounds__(64 * kKernelWaves) void k_kernel_pointgrad(int nrows, int rpad, int nsum, int spad, int dq, int diagonal,
                                                                        const double *__restrict__ rzt, const double *__restrict__ rnrm,
                                                                        const double *__restrict__ szt, const double *__restrict__ snrm,
                                                                        const double *__restrict__ U, const double *__restrict__ W, int mc, int tiles_per_slab,
                                                                        double *__restrict__ part) {
  using T = KernelTile<double, DQ>;
  constexpr int MQ = kKernelPointGradCols / 4;
  constexpr int NT = T::NT;
  constexpr int WPT = (16 * kKernelPointGradCols + NT - 1) / NT;
  __shared__ __attribute__((aligned(16))) double Ws[kKernelPointGradCols][16];
  __shared__ __attribute__((aligned(16))) double Zs[DQ * 4][16];
  __shared__ double Ns[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int i0 = blockIdx.x * kKernelRows + wave * 16;
  int t_begin, t_end;
  kernel_slab_tiles<int>(spad >> 4, tiles_per_slab, (int)blockIdx.y, &t_begin, &t_end);
  const int mq = (mc + 3) >> 2;

  // this wave's rows: z_I^T and U_I^T as B operands, |z_i|^2 for the lane's column i = lr
  double zi[DQ], ni, uc[MQ];
  T::rows(rzt, rnrm, rpad, dq, i0, lr, lk, zi, ni);
  const bool i_ok = i0 + lr < nrows;
#pragma unroll
  for (int q = 0; q < MQ; ++q) uc[q] = (i_ok && 4 * q + lk < mc) ? U[(int64_t)(4 * q + lk) * nrows + i0 + lr] : 0.0;
  double acc[DQ];
#pragma unroll
  for (int q = 0; q < DQ; ++q) acc[q] = 0.0;

  double wreg[WPT], zreg[T::ZPT], nreg = 0.0;
  auto fetch = [&](int t) {
    const int j0 = t * 16;
#pragma unroll
    for (int u = 0; u < WPT; ++u) {
      const int e = tid + u * NT, c = e >> 4, j = j0 + (e & 15);
      wreg[u] = (c < mc && j < nsum) ? W[(int64_t)c * nsum + j] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < T::ZPT; ++u) {
      const int e = tid + u * NT, k = e >> 4, jj = e & 15;
      zreg[u] = (e < DQ * 64 && k < 4 * dq) ? szt[(int64_t)k * spad + j0 + jj] : 0.0;
    }
    if (tid < 16) nreg = snrm[j0 + tid];
  };
  auto stash = [&]() {
#pragma unroll
    for (int u = 0; u < WPT; ++u) {
      const int e = tid + u * NT;
      if (e < 16 * kKernelPointGradCols) Ws[e >> 4][e & 15] = wreg[u];
    }
    T::stash(Zs, Ns, tid, zreg, nreg);
  };
  kernel_tile_walk(t_begin, t_end, fetch, stash, [&](int t) {
    const kd4_t g = T::gram(Zs, zi, dq, lr, lk);
    kd4_t c = (kd4_t)0.0;
#pragma unroll
    for (int q = 0; q < MQ; ++q)
      if (q < mq) c = kernel_mfma(Ws[4 * q + lk][lr], uc[q], c);
    double b[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool diag = diagonal && t * 16 + T::jr(lk, r) == i0 + lr;
      double phi, chi;
      kernel_profile_pair<double, PROFILE>(T::r2(g, r, ni, Ns, lk, diag), phi, chi);
      b[r] = chi * c[r];
    }
#pragma unroll
    for (int src = 0; src < 4; ++src)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double bj = __shfl(b[r], lr + 16 * src, 64);  // chi c of the pair (i = lr, j = src + 4 r)
#pragma unroll
        for (int q = 0; q < DQ; ++q)
          if (q < dq) acc[q] = fma(bj, zi[q] - Zs[4 * q + lk][src + 4 * r], acc[q]);
      }
  });
  if (i_ok) {
    const int dpad = 4 * dq;
    double *o = part + ((int64_t)blockIdx.y * nrows + i0 + lr) * dpad;
#pragma unroll
    for (int q = 0; q < DQ; ++q)
      if (q < dq) o[4 * q + lk] = acc[q];
  }
}

// One thread per value (a, k), k < d: the nslabs partials added in slab order, scaled by -s / l_k (s from the operator's device words,
// l from the host scale at update time), folded with alpha and beta. beta == 0 does not read vals.
__global__ __launch_bounds__(256) void k_kernel_pointgrad_sum(int64_t nrows, int d, int dpad, int nslabs, const double *__restrict__ part,
                                                              const double *__restrict__ params, KernelPointGradScale sc, double alpha, double beta,
                                                              double *__restrict__ vals) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= nrows * d) return;
  const int64_t a = e / d;
  const int k = (int)(e - a * d);
  const double *p = part + a * dpad + k;
  double v = p[0];
  for (int z = 1; z < nslabs; ++z) v += p[(int64_t)z * nrows * dpad];
  v *= -(params[0] / sc.ls[k]);
  const double old = beta == 0.0 ? 0.0 : beta * vals[e];
  vals[e] = fma(alpha, v, old);
}
#endif  // __HIPCC__ && SLQ_KERNELPOINTGRAD_DEVICE

}  // namespace slq
