// slq_kernelcross.hpp — cross-covariance products of the matrix-free kernel operator (slq_kernel_cross_*). For a
// kernel operator with points x_1..x_n (centre mean(x), lengthscales l, outputscale s, dtype F) and m NEW points x*_1..x*_m
//   z*_i = (F)(((double)x*_i - mean(x)) / l)        the TRAINING centre, double arithmetic, one rounding
//   r2_ij = max(0, fma(-2, z*_i.z_j, |z*_i|^2 + |z_j|^2))        no diagonal rule
//   C = s phi(r2)        m x n, no noise term
// and the two products Y = C W (forward: W n x b, Y m x b) and Y = C^T U (adjoint: U m x b, Y n x b). Both are ONE kernel with the
// two point sets exchanging roles: the "row" points own the output rows, the "summed" points are walked in tiles of 16. C is
// never held: k_kernel_panel's tile walk, on column-major operands with a leading dimension.
// Two parts:
//   host (plain C++, no HIP include; scripts/kernelcross_check.cpp runs it under the host sanitizers)
//     kernel_cross_schedule   row blocks, column chunks and slabs of the summed points for (nrows, nsum, b, num_cus)
//                             (slq_debug_kernel_cross_schedule)
//   device (hipcc only)
//     k_kernel_cross       Y (or one slab's partial of it) = s phi(r2) W
//     k_kernel_cross_sum   the slab partials summed in slab order
//   The instantiations of k_kernel_cross (2 dtypes x 4 profiles x 5 NCB x 2 DQ) live in slq_kernelcross.hip, a translation unit
//   of their own; slq.hip sees only kernel_cross_launch / kernel_cross_sum_launch.
#pragma once

#include "slq_kernelop.hpp"

namespace slq {

// Slabs of the summed points. The cost rule below has its optimum near sqrt(1 / 0.005) = 14 slabs for a single workgroup and
// below that for more, so the cap seldom binds; 64 (against kernel_schedule's 16) bounds the scratch - nslabs x nrows x b words -
// and the length of the schedule's array, and leaves the rule alone where a wide column range (b > 256: several workgroups per
// row block already) makes a round of workgroups fall just short of the chip.
constexpr int kKernelCrossMaxSlabs = 64;

// ---- the schedule of one product ------------------------------------------------------------------------------------------
// A workgroup owns kKernelRows output rows and 16 * col_blocks of the b columns (col_blocks the smallest of 1, 2, 4, 8, 16 that
// covers min(b, 256); further 256-column chunks along gridDim.y) and walks the summed points in tiles of 16. Few rows (a forward
// product with m = 128 new points is ONE row block): the summed range is cut into `nslabs` runs of whole tiles by kernel_schedule's
// cost rule - rounds of workgroups times the work of one, plus 0.005 per slab; slab z covers the summed points
// [slab_begin[z], slab_begin[z + 1]) = tiles [z * tiles_per_slab, (z + 1) * tiles_per_slab), lands in its own partial, and the
// partials are summed in slab order (no atomics). One slab writes the result directly.
struct KernelCrossSchedule {
  int rows_per_block = kKernelRows;
  int nrow_blocks = 0;
  int col_blocks = 0;   // 16-column tiles per workgroup: 1, 2, 4, 8 or 16
  int ncol_chunks = 0;  // gridDim.y
  int nslabs = 0;       // gridDim.z
  int tiles_per_slab = 0;
  int64_t slab_begin[kKernelCrossMaxSlabs + 1] = {};
};
inline KernelCrossSchedule kernel_cross_schedule(int64_t nrows, int64_t nsum, int64_t b, int num_cus) {
  KernelCrossSchedule S;
  S.nrow_blocks = (int)((nrows + kKernelRows - 1) / kKernelRows);
  const int want = (int)((std::min<int64_t>(b, 16 * kKernelMaxColBlocks) + 15) / 16);
  S.col_blocks = 1;
  while (S.col_blocks < want) S.col_blocks *= 2;
  S.ncol_chunks = (int)((b + 16 * kKernelMaxColBlocks - 1) / (16 * kKernelMaxColBlocks));  // (b <= 256: one chunk, whatever col_blocks)
  const int64_t ntiles = (nsum + 15) / 16;
  const double wgs = (double)S.nrow_blocks * S.ncol_chunks;
  double best = 1e300;
  int ks_best = 1;
  for (int ks = 1; ks <= kKernelCrossMaxSlabs && ks <= ntiles; ++ks) {
    const double cost = std::ceil(wgs * ks / std::max(num_cus, 1)) / ks + 0.005 * ks;
    if (cost < best - 1e-12) best = cost, ks_best = ks;
  }
  S.tiles_per_slab = (int)((ntiles + ks_best - 1) / ks_best);
  S.nslabs = (int)((ntiles + S.tiles_per_slab - 1) / S.tiles_per_slab);  // (no empty slab)
  for (int z = 0; z <= S.nslabs; ++z) S.slab_begin[z] = std::min<int64_t>(nsum, (int64_t)z * S.tiles_per_slab * 16);
  S.slab_begin[S.nslabs] = nsum;
  return S;
}
// the tiles [first, last) slab z of a launch walks: what k_kernel_cross computes from blockIdx.z and tiles_per_slab
inline void kernel_cross_slab_tiles(int64_t ntiles, int tiles_per_slab, int z, int64_t *first, int64_t *last) {
  *first = std::min<int64_t>(ntiles, (int64_t)z * tiles_per_slab);
  *last = std::min<int64_t>(ntiles, *first + tiles_per_slab);
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
bool kernel_cross_launch(int dtype_is_f64, int profile, const KernelCrossSchedule &S, const KernelCrossArgs &a, void *stream);
// Y[i + c ldy] = sum_z part[z * slab_stride + i + c nrows], z ascending
void kernel_cross_sum_launch(int dtype_is_f64, int64_t nrows, int b, int nslabs, const void *part, int64_t slab_stride, void *Y, int64_t ldy, void *stream);

#if defined(__HIPCC__) && defined(SLQ_KERNELCROSS_DEVICE)
// ---- device -------------------------------------------------------------------------------------------------------------
// Grid (row blocks, 256-column chunks, slabs); a wave owns 16 rows I and NCB 16-column tiles of the columns [col0, col0 + 16 NCB).
// Per tile J of 16 summed points, as k_kernel_panel:
//   G^T = z_J z_I^T   DQ MFMAs at most: A operand z_J from LDS (k-major), B operand z_I from registers (loaded once); the result
//                     puts C^T[j][i = lane & 15] in the lane that supplies C[i][j] as the A operand of the second product;
//   C = phi(r2)       4 values per lane, once per (i, j); r2 clamped at 0, NO diagonal rule (the two point sets are different sets);
//   acc += C W_J      4 NCB MFMAs, W_J (16 x 16 NCB) from LDS.
// The next tile's W, z and norms travel in registers while this tile computes. W is column-major: consecutive threads fetch
// consecutive j of one column (w_row / w_col below). Rows i >= nrows are computed on zero padding and never stored; points
// j >= nsum enter with W = 0 (phi is finite at the zero padding of z); columns g >= b likewise. The epilogue is s * acc: no
// sigma2 term. The order of j is fixed and nothing is atomic: identical calls give identical bits.
template <typename F, int PROFILE, int NCB, int DQ>
__global__ __launch_bounds__(64 * kKernelWaves) void k_kernel_cross(int nrows, int rpad, int nsum, int spad, int dq, const F *__restrict__ rzt,
                                                                    const F *__restrict__ rnrm, const F *__restrict__ szt, const F *__restrict__ snrm,
                                                                    const F *__restrict__ params, const F *__restrict__ W, int64_t ldw, int b,
                                                                    int tiles_per_slab, F *__restrict__ out, int64_t ldo, int64_t slab_stride) {
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
  const int col0 = blockIdx.y * (16 * kKernelMaxColBlocks);
  const int i0 = blockIdx.x * kKernelRows + wave * 16;
  const int ntiles = spad >> 4;
  const int t_begin = min(ntiles, (int)blockIdx.z * tiles_per_slab), t_end = min(ntiles, t_begin + tiles_per_slab);

  // this wave's rows: z_I^T as the B operand of the first product, |z_i|^2 for the lane's column i = lr
  F zi[DQ];
  const bool i_ok = i0 + lr < rpad;
#pragma unroll
  for (int q = 0; q < DQ; ++q) zi[q] = (q < dq && i_ok) ? rzt[(int64_t)(4 * q + lk) * rpad + i0 + lr] : (F)0;
  const F ni = i_ok ? rnrm[i0 + lr] : (F)0;
  V4 acc[NCB];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) acc[cb] = (V4)(F)0;

  // element e of the 16 x NC tile of W -> (row jj, column c). W is column-major, so a thread run should stay in one column; the LDS
  // store wants a wave's 64 elements on distinct banks. fp32 (row stride NC + 4 words): 16 rows x 4 columns per wave do both. fp64
  // (row stride = 32 words mod 64): that shape would put 8 rows on one bank; 4 rows x 16 columns per wave - 32-byte runs of a column -
  // is two lanes per bank, what a 512-byte store costs anyway.
  auto w_row = [](int e) { return F64 ? ((e & 3) | ((e >> 4) & 12)) : (e & 15); };
  auto w_col = [](int e) { return F64 ? (((e >> 2) & 15) | ((e >> 8) << 4)) : (e >> 4); };
  F wreg[WPT], zreg[ZPT], nreg = (F)0;
  auto fetch = [&](int t) {
    const int j0 = t * 16;
#pragma unroll
    for (int u = 0; u < WPT; ++u) {
      const int e = tid + u * NT, c = w_col(e), j = j0 + w_row(e);
      const int g = col0 + c;
      F v = (F)0;
      if (e < 16 * NC && j < nsum && g < b) v = W[(int64_t)g * ldw + j];
      wreg[u] = v;
    }
#pragma unroll
    for (int u = 0; u < ZPT; ++u) {
      const int e = tid + u * NT, k = e >> 4, jj = e & 15;
      zreg[u] = (e < DQ * 64 && k < 4 * dq) ? szt[(int64_t)k * spad + j0 + jj] : (F)0;
    }
    if (tid < 16) nreg = snrm[j0 + tid];
  };
  auto stash = [&]() {
#pragma unroll
    for (int u = 0; u < WPT; ++u) {
      const int e = tid + u * NT;
      if (e < 16 * NC) Ws[w_row(e)][w_col(e)] = wreg[u];
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
  const F s = params[0];
  F *o = out + (int64_t)blockIdx.z * slab_stride;
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) {
    const int g = col0 + cb * 16 + lr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + (F64 ? lk + 4 * r : 4 * lk + r);
      if (i < nrows && g < b) o[(int64_t)g * ldo + i] = s * acc[cb][r];
    }
  }
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

// the launch for (dtype, profile, schedule, d): every instantiation is named here
template <typename F, int PROFILE, int NCB> static inline void kernel_cross_launch_dq(const KernelCrossSchedule &S, const KernelCrossArgs &a, hipStream_t st) {
  const dim3 g(S.nrow_blocks, S.ncol_chunks, S.nslabs), blk(64 * kKernelWaves);
  if (a.dq <= 4)
    k_kernel_cross<F, PROFILE, NCB, 4><<<g, blk, 0, st>>>(a.nrows, a.rpad, a.nsum, a.spad, a.dq, (const F *)a.rzt, (const F *)a.rnrm, (const F *)a.szt, (const F *)a.snrm,
                                                        (const F *)a.params, (const F *)a.W, a.ldw, a.b, S.tiles_per_slab, (F *)a.out, a.ldo, a.slab_stride);
  else
    k_kernel_cross<F, PROFILE, NCB, 16><<<g, blk, 0, st>>>(a.nrows, a.rpad, a.nsum, a.spad, a.dq, (const F *)a.rzt, (const F *)a.rnrm, (const F *)a.szt, (const F *)a.snrm,
                                                         (const F *)a.params, (const F *)a.W, a.ldw, a.b, S.tiles_per_slab, (F *)a.out, a.ldo, a.slab_stride);
}
template <typename F, int PROFILE> static inline bool kernel_cross_launch_ncb(const KernelCrossSchedule &S, const KernelCrossArgs &a, hipStream_t st) {
  switch (S.col_blocks) {
    case 1: kernel_cross_launch_dq<F, PROFILE, 1>(S, a, st); return true;
    case 2: kernel_cross_launch_dq<F, PROFILE, 2>(S, a, st); return true;
    case 4: kernel_cross_launch_dq<F, PROFILE, 4>(S, a, st); return true;
    case 8: kernel_cross_launch_dq<F, PROFILE, 8>(S, a, st); return true;
    case 16: kernel_cross_launch_dq<F, PROFILE, 16>(S, a, st); return true;
    default: return false;
  }
}
template <typename F> static inline bool kernel_cross_launch_profile(int profile, const KernelCrossSchedule &S, const KernelCrossArgs &a, hipStream_t st) {
  switch (profile) {
    case KERNEL_RBF: return kernel_cross_launch_ncb<F, KERNEL_RBF>(S, a, st);
    case KERNEL_MATERN12: return kernel_cross_launch_ncb<F, KERNEL_MATERN12>(S, a, st);
    case KERNEL_MATERN32: return kernel_cross_launch_ncb<F, KERNEL_MATERN32>(S, a, st);
    case KERNEL_MATERN52: return kernel_cross_launch_ncb<F, KERNEL_MATERN52>(S, a, st);
    default: return false;
  }
}
#endif  // __HIPCC__ && SLQ_KERNELCROSS_DEVICE

}  // namespace slq
