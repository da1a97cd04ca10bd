// slq_kernelfeatureadj.hpp — the adjoint of the random-feature map of slq_kernelfeature.hpp (slq_kernel_feature_rmatmat / _rdmat;
// DESIGN.md §4.22). With the row points z_i, the frequencies Omega, g_ij = sum_k Omega_jk z_ik and a = sqrt(s / F2) of that header
//   Z[j, c] = a sum_i cos g_ij U[i, c],     Z[F2 + j, c] = a sum_i sin g_ij U[i, c]
// for a column-major U (nrows x b); Z is 2 F2 x b, its row order that of the forward product's W. The walk is that of
// slq_kerneltile.hpp with the roles exchanged: the "row" set is the frequencies (a workgroup owns 128 of them, Omega_I in registers
// as the B operand), the "summed" set is the row points, whose z^T tiles of 16 go through LDS; G^T = z_J Omega_I^T is
// KernelTile::gram, and the second product feeds two accumulator sets, one per half of Z. Phi is never held.
//   host (plain C++, no HIP include; scripts/kernelfeatureadj_check.cpp runs it under the host sanitizers)
//     kernel_feature_adjoint_schedule   row blocks of the frequencies, column chunks and slabs of the row points for
//                                       (F2, nrows, b, num_cus): kernel_cross_schedule with F2 as the row count, 128-column
//                                       chunks in fp64 and the adjoint's own price of a slab; the slab partials (2 F2 x b each) are summed in slab order by
//                                       k_kernel_cross_sum
//   device (hipcc only)
//     kernel_feature_adjoint_product    the body
//     k_kernel_feature_adjoint          its kernel: (5 NCB in fp32 + 4 in fp64) x 2 DQ in slq_kernelfeatureadj.hip, a unit of its own
#pragma once

#include "slq_kernelfeature.hpp"

namespace slq {

// Two accumulator sets: fp64 with 16 column tiles would be 128 fp64 accumulators per lane, all 256 registers of a wave before any
// fragment (the compiler spills: 468 bytes of scratch per lane), so an fp64 workgroup takes at most 8 tiles and the column chunks are
// 128 wide; fp32 with 16 tiles fits (207 and 223 VGPRs, scratch 0) and keeps the cross product's 256
// (profiles/kernelfeature_adjoint_resources.txt).
constexpr int kKernelFeatureAdjMaxColBlocksF64 = 8;
inline int kernel_feature_adjoint_chunk_cols(bool f64) { return 16 * (f64 ? kKernelFeatureAdjMaxColBlocksF64 : kKernelMaxColBlocks); }

// The slabs of the row points: the cost rule of kernel_slab_split - rounds of workgroups times the work of one, plus a price per
// slab - with the adjoint's own price. kernel_slab_split's 0.005 is the cross product's; a tile of the adjoint is twice the MFMAs and a
// sincos per pair, so a slab's partial and its share of the sum weigh less against it: with 0.005 the common shape (F2 = 1024: 8 row
// blocks; n = 16384, b = 64) took 14 slabs, 112 workgroups and 0.263 ms against the forward product's 0.136; with 0.001 it takes 32
// slabs, one round of 256 workgroups, and 0.141 ms (0.0005 to 0.0001: the same 32). profiles/gp_features_bench.json.
constexpr double kKernelFeatureAdjSlabCost = 0.001;
inline KernelSlabSplit kernel_feature_adjoint_slab_split(int64_t ntiles, double wgs, int num_cus) {
  double best = 1e300;
  int ks_best = 1;
  for (int ks = 1; ks <= kKernelCrossMaxSlabs && ks <= ntiles; ++ks) {
    const double cost = std::ceil(wgs * ks / std::max(num_cus, 1)) / ks + kKernelFeatureAdjSlabCost * ks;
    if (cost < best - 1e-12) best = cost, ks_best = ks;
  }
  KernelSlabSplit s;
  s.tiles_per_slab = (int)((ntiles + ks_best - 1) / ks_best);
  s.nslabs = (int)((ntiles + s.tiles_per_slab - 1) / s.tiles_per_slab);  // (no empty slab)
  return s;
}

// kernel_cross_schedule for nfreq "row" frequencies, nrows summed row points and b columns: its row blocks and column tiles, in fp64
// with the narrower chunk, and the slabs of the adjoint's own rule for the workgroups that makes (at most kKernelCrossMaxSlabs: the
// length of the schedule's array).
inline KernelSchedule kernel_feature_adjoint_schedule(int64_t nfreq, int64_t nrows, int64_t b, int num_cus, bool f64) {
  KernelSchedule S = kernel_cross_schedule(nfreq, nrows, b, num_cus);
  if (f64 && S.col_blocks > kKernelFeatureAdjMaxColBlocksF64) {
    const int chunk = kernel_feature_adjoint_chunk_cols(true);
    S.col_blocks = kKernelFeatureAdjMaxColBlocksF64;
    S.ncol_chunks = (int)((b + chunk - 1) / chunk);
  }
  const KernelSlabSplit s = kernel_feature_adjoint_slab_split((nrows + 15) / 16, (double)S.nrow_blocks * S.ncol_chunks, num_cus);
  S.nslabs = s.nslabs, S.tiles_per_slab = s.tiles_per_slab;
  for (int z = 0; z <= kKernelCrossMaxSlabs; ++z) S.slab_begin[z] = 0;
  kernel_slab_begin(s, nrows, S.slab_begin);
  return S;
}

// what a launch reads and writes (plain pointers: the launch function is defined in slq_kernelfeatureadj.hip and called from slq.hip)
struct KernelFeatureAdjArgs {
  int nfreq, fpad;     // frequencies: F2, F2 rounded up to 16
  int nrows, rpad;     // row points: count, count rounded up to 16
  int dq;              // dpad / 4
  const void *omt;     // Omega transposed (dpad x fpad, k-major), zeros in the padding
  const void *rzt;     // row points: z transposed (dpad x rpad), zeros in the padding
  const void *params;  // {s, sigma2} of the operator, on the device; only s is read
  const void *U;       // nrows x b, column-major
  int64_t ldu;
  int b;
  void *out;  // nslabs == 1: Z (2 F2 x b, column-major, ldo); else the partials, slab z at out + z * slab_stride, ldo == 2 F2
  int64_t ldo, slab_stride;
};
// false: no such kernel (the caller reports it: there is no fallback). `stream` is a hipStream_t.
bool kernel_feature_adjoint_launch(int dtype_is_f64, const KernelSchedule &S, const KernelFeatureAdjArgs &a, void *stream);

#if defined(__HIPCC__) && defined(SLQ_KERNELFEATURE_DEVICE)
// ---- device -------------------------------------------------------------------------------------------------------------
// Z = a [cos(G) | sin(G)]^T U. Grid (row blocks of the frequencies, column chunks, slabs of the row points); a wave owns 16
// frequencies I and NCB 16-column tiles of the columns [col0, col0 + 16 NCB). Per tile J of 16 row points: G^T of KernelTile;
// cos and sin of the 4 values a lane holds (kernel_sincos: the accurate functions), once per (i, j), whatever NCB is;
// accC += cos U_J, accS += sin U_J, 8 NCB MFMAs, the one 16 x 16 NCB tile of U from LDS, staged once per workgroup by the column
// layout's map. Points i >= nrows are zero padding of z^T (cos 0 = 1) and enter with U = 0: the fetch is guarded and nothing past
// nrows is read; frequencies j >= F2 are computed on zero padding and never stored; columns g >= ncols likewise. a comes from
// params (device memory: a captured graph sees a hyperparameter change). gridDim.z > 1: slab z of the raw partial products at
// out + z * slab_stride. The order of i is fixed and nothing is atomic: identical calls give identical bits.
template <typename F, int NCB, int DQ>
__device__ __forceinline__ void kernel_feature_adjoint_product(int nfreq, int fpad, int nrows, int rpad, int dq, const F *omt, const F *rzt, const F *params,
                                                               const F *U, int64_t ldu, int ncols, int tiles_per_slab, F *out, int64_t ldo, int64_t slab_stride) {
  using T = KernelTile<F, DQ>;
  using V4 = typename T::V4;
  using L = KernelColumnLayout;
  constexpr bool F64 = T::F64;
  constexpr int NC = 16 * NCB;
  constexpr int WS = NC + (F64 ? (NC % 32 == 16 ? 0 : 16) : 4);  // row stride of the U tile: the 4 rows a read touches on distinct banks
  constexpr int NT = T::NT;
  constexpr int UPT = (16 * NC + NT - 1) / NT;  // U elements per thread and tile
  __shared__ __attribute__((aligned(16))) F Us[16][WS];
  __shared__ __attribute__((aligned(16))) F Zs[DQ * 4][16];
  __shared__ F Ns[16];  // (KernelTile::stash writes it; never read here)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int col0 = blockIdx.y * (F64 ? 16 * kKernelFeatureAdjMaxColBlocksF64 : 16 * kKernelMaxColBlocks);  // (kernel_feature_adjoint_chunk_cols)
  const int i0 = blockIdx.x * kKernelRows + wave * 16;
  int t_begin, t_end;
  kernel_slab_tiles<int>(rpad >> 4, tiles_per_slab, (int)blockIdx.z, &t_begin, &t_end);

  // the wave's frequencies i0 .. i0 + 15: Omega_I^T as the B operand of the first product (KernelTile::rows without the norms:
  // the frequencies have none)
  F zi[DQ];
  {
    const bool i_ok = i0 + lr < fpad;
#pragma unroll
    for (int q = 0; q < DQ; ++q) zi[q] = (q < dq && i_ok) ? omt[(int64_t)(4 * q + lk) * fpad + i0 + lr] : (F)0;
  }
  V4 accC[NCB], accS[NCB];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) accC[cb] = (V4)(F)0, accS[cb] = (V4)(F)0;

  F ureg[UPT], zreg[T::ZPT];
  auto fetch = [&](int t) {
    const int j0 = t * 16;
#pragma unroll
    for (int u = 0; u < UPT; ++u) {
      const int e = tid + u * NT, c = L::template w_col<F, NC>(e), j = j0 + L::template w_row<F, NC>(e);
      const int g = col0 + c;
      F v = (F)0;
      if (e < 16 * NC && j < nrows && g < ncols) v = U[(int64_t)g * ldu + j];
      ureg[u] = v;
    }
#pragma unroll
    for (int u = 0; u < T::ZPT; ++u) {
      const int e = tid + u * NT, k = e >> 4, jj = e & 15;
      zreg[u] = (e < DQ * 64 && k < 4 * dq) ? rzt[(int64_t)k * rpad + j0 + jj] : (F)0;
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int u = 0; u < UPT; ++u) {
      const int e = tid + u * NT;
      if (e < 16 * NC) Us[L::template w_row<F, NC>(e)][L::template w_col<F, NC>(e)] = ureg[u];
    }
    T::stash(Zs, Ns, tid, zreg, (F)0);
  };
  kernel_tile_walk(t_begin, t_end, fetch, stash, [&](int) {
    const V4 g = T::gram(Zs, zi, dq, lr, lk);
    F cs[4], sn[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) kernel_sincos(g[r], sn[r], cs[r]);
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const F u = Us[T::jr(lk, r)][cb * 16 + lr];
        accC[cb] = kernel_mfma(cs[r], u, accC[cb]);
        accS[cb] = kernel_mfma(sn[r], u, accS[cb]);
      }
  });
  const F a = sqrt(params[0] / (F)nfreq);
  F *o = out + (int64_t)blockIdx.z * slab_stride;
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) {
    const int g = col0 + cb * 16 + lr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + T::jr(lk, r);
      if (i < nfreq && g < ncols) {
        const int64_t off = (int64_t)g * ldo + i;
        o[off] = a * accC[cb][r], o[off + nfreq] = a * accS[cb][r];
      }
    }
  }
}

template <typename F, int NCB, int DQ>
__global__ __launch_bounds__(64 * kKernelWaves) void k_kernel_feature_adjoint(int nfreq, int fpad, int nrows, int rpad, int dq, const F *__restrict__ omt,
                                                                              const F *__restrict__ rzt, const F *__restrict__ params, const F *__restrict__ U,
                                                                              int64_t ldu, int b, int tiles_per_slab, F *__restrict__ out, int64_t ldo,
                                                                              int64_t slab_stride) {
  kernel_feature_adjoint_product<F, NCB, DQ>(nfreq, fpad, nrows, rpad, dq, omt, rzt, params, U, ldu, b, tiles_per_slab, out, ldo, slab_stride);
}

template <typename F> static inline bool kernel_feature_adjoint_launch_dtype(const KernelSchedule &S, const KernelFeatureAdjArgs &a, hipStream_t st) {
  const dim3 g(S.nrow_blocks, S.ncol_chunks, S.nslabs), blk(64 * kKernelWaves);
  return kernel_for_ncb(S.col_blocks, [&](auto NCB) {
    return kernel_for_dq(a.dq, [&](auto DQ) {
      if constexpr (sizeof(F) == 8 && NCB() > kKernelFeatureAdjMaxColBlocksF64) return false;
      else {
      k_kernel_feature_adjoint<F, NCB(), DQ()><<<g, blk, 0, st>>>(a.nfreq, a.fpad, a.nrows, a.rpad, a.dq, (const F *)a.omt, (const F *)a.rzt, (const F *)a.params,
                                                                (const F *)a.U, a.ldu, a.b, S.tiles_per_slab, (F *)a.out, a.ldo, a.slab_stride);
      return true;
      }
    });
  });
}
#endif  // __HIPCC__ && SLQ_KERNELFEATURE_DEVICE

}  // namespace slq
