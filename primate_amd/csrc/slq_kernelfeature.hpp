// slq_kernelfeature.hpp — random Fourier features of the kernel operator's stationary profile (slq_kernel_feature_*; DESIGN.md
// §4.21). For row points z_i (the operator's own z, or the z* of a slq_kernel_cross), F2 frequencies Omega (F2 x d, rounded once to
// the dtype F) and the outputscale s
//   g_ij = sum_k Omega_jk z_ik
//   Y_ic = a sum_j (cos g_ij W[j, c] + sin g_ij W[F2 + j, c]),     a = sqrt(s / F2) in F from params[0] on the device
// for a column-major W (2 F2 x b). The profile lives in the law Omega was drawn from (Student-t for the Matern family), so the
// kernel has no profile parameter. The walk is that of slq_kerneltile.hpp with the frequencies in the place of the summed points:
// G^T = Omega_J z_I^T is KernelTile::gram, cos and sin take the place of the profile (no norms, no r2, no clamp), and the second
// product accumulates both halves of W into the same accumulators. Phi is never held.
//   host (plain C++, no HIP include; scripts/kernelfeature_check.cpp runs it under the host sanitizers)
//     kernel_feature_schedule   row blocks, column chunks and slabs of the frequencies for (nrows, F2, b, num_cus):
//                               kernel_cross_schedule, with 128-column chunks in fp64; the slab partials are summed in slab
//                               order by k_kernel_cross_sum
//   device (hipcc only)
//     kernel_feature_product    the body, beside kernel_product
//     k_kernel_feature          its kernel: (5 NCB in fp32 + 4 in fp64) x 2 DQ instantiations in slq_kernelfeature.hip, a unit of its own
#pragma once

#include "slq_kernelcross.hpp"

namespace slq {

constexpr int64_t kKernelFeatureMaxFreq = (int64_t)1 << 30;  // 2 F2 rows of W are indexed in 32 bits next to a tile offset

// fp64 with 16 column tiles does not fit its registers (two staged halves of W on top of 64 accumulators: the compiler spills), so an
// fp64 workgroup takes at most 8 tiles and the column chunks are 128 wide; fp32 keeps the cross product's 256
// (profiles/kernelfeature_resources.txt).
constexpr int kKernelFeatureMaxColBlocksF64 = 8;
inline int kernel_feature_chunk_cols(bool f64) { return 16 * (f64 ? kKernelFeatureMaxColBlocksF64 : kKernelMaxColBlocks); }

// kernel_cross_schedule for nrows row points, F2 "summed" frequencies and b columns; in fp64 with the narrower chunk, the slabs
// chosen again for the workgroups that makes
inline KernelSchedule kernel_feature_schedule(int64_t nrows, int64_t nfreq, int64_t b, int num_cus, bool f64) {
  KernelSchedule S = kernel_cross_schedule(nrows, nfreq, b, num_cus);
  if (f64 && S.col_blocks > kKernelFeatureMaxColBlocksF64) {
    const int chunk = kernel_feature_chunk_cols(true);
    S.col_blocks = kKernelFeatureMaxColBlocksF64;
    S.ncol_chunks = (int)((b + chunk - 1) / chunk);
    const KernelSlabSplit s = kernel_slab_split((nfreq + 15) / 16, (double)S.nrow_blocks * S.ncol_chunks, num_cus, kKernelCrossMaxSlabs);
    S.nslabs = s.nslabs, S.tiles_per_slab = s.tiles_per_slab;
    for (int z = 0; z <= kKernelCrossMaxSlabs; ++z) S.slab_begin[z] = 0;
    kernel_slab_begin(s, nfreq, S.slab_begin);
  }
  return S;
}

// what a launch reads and writes (plain pointers: the launch function is defined in slq_kernelfeature.hip and called from slq.hip)
struct KernelFeatureArgs {
  int nrows, rpad;         // row points: count, count rounded up to 16
  int nfreq, fpad;         // frequencies: F2, F2 rounded up to 16
  int dq;                  // dpad / 4
  const void *rzt, *rnrm;  // row points: z transposed (dpad x rpad), |z|^2 (rpad; the arrays k_kernel_cross reads - the norms are not used)
  const void *omt;         // Omega transposed (dpad x fpad, k-major), zeros in the padding
  const void *params;      // {s, sigma2} of the operator, on the device; only s is read
  const void *W;           // 2 F2 x b, column-major: rows [0, F2) weigh the cosines, [F2, 2 F2) the sines
  int64_t ldw;
  int b;
  void *out;  // nslabs == 1: Y (nrows x b, column-major, ldo); else the partials, slab z at out + z * slab_stride, ldo == nrows
  int64_t ldo, slab_stride;
};
// false: no such kernel (the caller reports it: there is no fallback). `stream` is a hipStream_t.
bool kernel_feature_launch(int dtype_is_f64, const KernelSchedule &S, const KernelFeatureArgs &a, void *stream);

#if defined(__HIPCC__) && defined(SLQ_KERNELFEATURE_DEVICE)
// ---- device -------------------------------------------------------------------------------------------------------------
// sin and cos with full range reduction (the device library's accurate functions: matern12 frequencies are Cauchy and |g| reaches
// 1e3 - 1e4; no native approximation)
__device__ __forceinline__ void kernel_sincos(double g, double &sn, double &cs) { sincos(g, &sn, &cs); }
__device__ __forceinline__ void kernel_sincos(float g, float &sn, float &cs) { sincosf(g, &sn, &cs); }

// Y = a (cos(G) W_c + sin(G) W_s). Grid (row blocks, column chunks, slabs); a wave owns 16 rows I and NCB 16-column tiles of the
// columns [col0, col0 + 16 NCB). Per tile J of 16 frequencies: G^T of KernelTile; cos and sin of the 4 values a lane holds, once
// per (i, j), whatever NCB is; acc += cos W_cJ + sin W_sJ, 8 NCB MFMAs, the two 16 x 16 NCB tiles of W (rows j and F2 + j) from LDS,
// staged once per workgroup by the column layout's map. Rows i >= nrows are computed on zero padding and never stored; frequencies
// j >= F2 are zero padding (cos 0 = 1) and enter with W = 0 in both halves; columns g >= ncols likewise. a comes from params
// (device memory: a captured graph sees a hyperparameter change). gridDim.z > 1: slab z of the raw partial products at
// out + z * slab_stride. The order of j is fixed and nothing is atomic: identical calls give identical bits.
template <typename F, int NCB, int DQ>
__device__ __forceinline__ void kernel_feature_product(int nrows, int rpad, int nfreq, int fpad, int dq, const F *rzt, const F *rnrm, const F *omt,
                                                       const F *params, const F *W, int64_t ldw, int ncols, int tiles_per_slab, F *out, int64_t ldo,
                                                       int64_t slab_stride) {
  using T = KernelTile<F, DQ>;
  using V4 = typename T::V4;
  using L = KernelColumnLayout;
  constexpr bool F64 = T::F64;
  constexpr int NC = 16 * NCB;
  constexpr int WS = NC + (F64 ? (NC % 32 == 16 ? 0 : 16) : 4);  // row stride of a W tile: the 4 rows a read touches on distinct banks
  constexpr int NT = T::NT;
  constexpr int WPT = (16 * NC + NT - 1) / NT;  // elements per thread, tile and half of W
  __shared__ __attribute__((aligned(16))) F Wc[16][WS];
  __shared__ __attribute__((aligned(16))) F Wn[16][WS];
  __shared__ __attribute__((aligned(16))) F Zs[DQ * 4][16];
  __shared__ F Ns[16];  // (KernelTile::stash writes it; never read here)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int col0 = blockIdx.y * (F64 ? 16 * kKernelFeatureMaxColBlocksF64 : 16 * kKernelMaxColBlocks);  // (kernel_feature_chunk_cols)
  const int i0 = blockIdx.x * kKernelRows + wave * 16;
  int t_begin, t_end;
  kernel_slab_tiles<int>(fpad >> 4, tiles_per_slab, (int)blockIdx.z, &t_begin, &t_end);

  F zi[DQ], ni;
  T::rows(rzt, rnrm, rpad, dq, i0, lr, lk, zi, ni);
  V4 acc[NCB];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) acc[cb] = (V4)(F)0;

  F creg[WPT], sreg[WPT], zreg[T::ZPT];
  auto fetch = [&](int t) {
    const int j0 = t * 16;
#pragma unroll
    for (int u = 0; u < WPT; ++u) {
      const int e = tid + u * NT, c = L::template w_col<F, NC>(e), j = j0 + L::template w_row<F, NC>(e);
      const int g = col0 + c;
      F vc = (F)0, vs = (F)0;
      if (e < 16 * NC && j < nfreq && g < ncols) {
        const int64_t off = (int64_t)g * ldw + j;
        vc = W[off], vs = W[off + nfreq];
      }
      creg[u] = vc, sreg[u] = vs;
    }
#pragma unroll
    for (int u = 0; u < T::ZPT; ++u) {
      const int e = tid + u * NT, k = e >> 4, jj = e & 15;
      zreg[u] = (e < DQ * 64 && k < 4 * dq) ? omt[(int64_t)k * fpad + j0 + jj] : (F)0;
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int u = 0; u < WPT; ++u) {
      const int e = tid + u * NT;
      if (e < 16 * NC) {
        const int r = L::template w_row<F, NC>(e), c = L::template w_col<F, NC>(e);
        Wc[r][c] = creg[u], Wn[r][c] = sreg[u];
      }
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
        acc[cb] = kernel_mfma(cs[r], Wc[T::jr(lk, r)][cb * 16 + lr], acc[cb]);
        acc[cb] = kernel_mfma(sn[r], Wn[T::jr(lk, r)][cb * 16 + lr], acc[cb]);
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
      if (i < nrows && g < ncols) o[(int64_t)g * ldo + i] = a * acc[cb][r];
    }
  }
}

template <typename F, int NCB, int DQ>
__global__ __launch_bounds__(64 * kKernelWaves) void k_kernel_feature(int nrows, int rpad, int nfreq, int fpad, int dq, const F *__restrict__ rzt,
                                                                      const F *__restrict__ rnrm, const F *__restrict__ omt, const F *__restrict__ params,
                                                                      const F *__restrict__ W, int64_t ldw, int b, int tiles_per_slab, F *__restrict__ out,
                                                                      int64_t ldo, int64_t slab_stride) {
  kernel_feature_product<F, NCB, DQ>(nrows, rpad, nfreq, fpad, dq, rzt, rnrm, omt, params, W, ldw, b, tiles_per_slab, out, ldo, slab_stride);
}

template <typename F> static inline bool kernel_feature_launch_dtype(const KernelSchedule &S, const KernelFeatureArgs &a, hipStream_t st) {
  const dim3 g(S.nrow_blocks, S.ncol_chunks, S.nslabs), blk(64 * kKernelWaves);
  return kernel_for_ncb(S.col_blocks, [&](auto NCB) {
    return kernel_for_dq(a.dq, [&](auto DQ) {
      if constexpr (sizeof(F) == 8 && NCB() > kKernelFeatureMaxColBlocksF64) return false;
      else {
      k_kernel_feature<F, NCB(), DQ()><<<g, blk, 0, st>>>(a.nrows, a.rpad, a.nfreq, a.fpad, a.dq, (const F *)a.rzt, (const F *)a.rnrm, (const F *)a.omt,
                                                        (const F *)a.params, (const F *)a.W, a.ldw, a.b, S.tiles_per_slab, (F *)a.out, a.ldo, a.slab_stride);
      return true;
      }
    });
  });
}
#endif  // __HIPCC__ && SLQ_KERNELFEATURE_DEVICE

}  // namespace slq
