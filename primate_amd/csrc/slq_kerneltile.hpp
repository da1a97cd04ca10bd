// slq_kerneltile.hpp — what the kernels of the matrix-free kernel operator share, stated once: the product
// (slq_kernelop.hpp), the hyperparameter gradients (slq_kernelgrad.hpp) and the cross-covariance products (slq_kernelcross.hpp)
// are ONE walk. A workgroup of kKernelWaves waves owns kKernelRows "row" points, 16 per wave, and walks the "summed" points in
// tiles of 16; per tile the scaled squared distances r2 of the 16 x 16 pairs come from a small MFMA GEMM of the coordinates and
// stay in the registers they were computed in. That the three kernels form r2 from the same operands in the same order is a
// contract - the gradient carries the operator's bits, a cross product over the training points equals the operator's product
// bit for bit - and this header is where it is kept.
// Two parts:
//   host (plain C++, no HIP include; scripts/kernel*_check.cpp run it under the host sanitizers)
//     kernel_slab_split       how many slabs the summed points are cut into: the cost rule
//     kernel_slab_tiles       the tiles slab z walks (host and device: the schedules and the kernels share the statement)
//     kernel_slab_begin       slab_begin[] of a schedule from the split
//     kernel_product_schedule row blocks, column chunks and slabs of one product (KernelSchedule)
//   device (hipcc only)
//     kernel_profile_pair, kernel_profile   phi and chi = -2 dphi/dr2 of the four profiles
//     KernelTile              the z tile and the norms of the summed points in LDS, the row points' fragments, G^T and r2
//     kernel_tile_walk        the double-buffered loop over a slab's tiles
//     kernel_product          Y = s phi(r2) W (+ sigma2 W) for a Layout of W and Y: the body of k_kernel_panel, k_kernel_panel_scaled and k_kernel_cross
//     kernel_for_profile / _ncb / _dq   the launch ladder: a run-time (profile, column tiles, depth) to its instantiation
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <type_traits>

#ifdef __HIPCC__
#define SLQ_KERNEL_HD __host__ __device__
#else
#define SLQ_KERNEL_HD
#endif

namespace slq {

constexpr int kKernelMaxDim = 64;        // d <= 64: the z fragments of a wave's rows live in registers
constexpr int kKernelWaves = 8;          // waves per workgroup
constexpr int kKernelRows = 16 * kKernelWaves;  // output rows per workgroup: 16 per wave
constexpr int kKernelMaxColBlocks = 16;  // 16-column accumulator tiles per wave: 256 columns, 64 fp64 accumulators per lane
constexpr int kKernelMaxSlabs = 16;      // slabs of the operator's product and of a gradient update (summed in slab order by k_3term_slabs)
// Slabs of a cross product. The cost rule has its optimum near sqrt(1 / 0.005) = 14 slabs for a single workgroup and below that
// for more, so the cap seldom binds; 64 bounds the scratch - nslabs x nrows x b words - and the length of the schedule's array,
// and leaves the rule alone where a wide column range (b > 256: several workgroups per row block already) makes a round of
// workgroups fall just short of the chip.
constexpr int kKernelCrossMaxSlabs = 64;

enum { KERNEL_RBF = 0, KERNEL_MATERN12 = 1, KERNEL_MATERN32 = 2, KERNEL_MATERN52 = 3, kNumKernelProfiles = 4 };

// ---- slabs ------------------------------------------------------------------------------------------------------------------
// Few row blocks do not fill the chip, so the summed points are also cut into `nslabs` runs of whole tiles, each landing in a
// partial of its own; the partials are summed in slab order (no atomics). nslabs minimises rounds of workgroups times the work
// of one, plus a small cost per slab - the rule of the dense operator's K split. The slab boundaries fix the summation order and
// therefore the bits.
struct KernelSlabSplit {
  int nslabs = 1, tiles_per_slab = 0;
};
inline KernelSlabSplit kernel_slab_split(int64_t ntiles, double wgs, int num_cus, int max_slabs) {
  double best = 1e300;
  int ks_best = 1;
  for (int ks = 1; ks <= max_slabs && ks <= ntiles; ++ks) {
    const double cost = std::ceil(wgs * ks / std::max(num_cus, 1)) / ks + 0.005 * ks;
    if (cost < best - 1e-12) best = cost, ks_best = ks;
  }
  KernelSlabSplit s;
  s.tiles_per_slab = (int)((ntiles + ks_best - 1) / ks_best);
  s.nslabs = (int)((ntiles + s.tiles_per_slab - 1) / s.tiles_per_slab);  // (no empty slab)
  return s;
}
// the tiles [first, last) slab z walks: what every kernel computes from its slab index and tiles_per_slab
template <typename I> SLQ_KERNEL_HD inline void kernel_slab_tiles(I ntiles, int tiles_per_slab, int z, I *first, I *last) {
  using std::min;
  *first = min(ntiles, (I)z * tiles_per_slab), *last = min(ntiles, *first + tiles_per_slab);
}
// slab z covers the points [slab_begin[z], slab_begin[z + 1]) of the npoints summed ones
inline void kernel_slab_begin(const KernelSlabSplit &s, int64_t npoints, int64_t *slab_begin) {
  for (int z = 0; z <= s.nslabs; ++z) slab_begin[z] = std::min<int64_t>(npoints, (int64_t)z * s.tiles_per_slab * 16);
  slab_begin[s.nslabs] = npoints;
}

// ---- the schedule of one product ----------------------------------------------------------------------------------------------
// A workgroup owns kKernelRows output rows and 16 * col_blocks of the ncols columns (col_blocks the smallest of 1, 2, 4, 8, 16
// that covers min(ncols, 256): the K tile is evaluated once for both panels of a 256-probe fp64 plan; further 256-column chunks
// along gridDim.y) and walks the nsum summed points in tiles of 16, slab z (gridDim.z) the tiles of kernel_slab_tiles.
struct KernelSchedule {
  int rows_per_block = kKernelRows;
  int nrow_blocks = 0;
  int col_blocks = 0;   // 16-column tiles per workgroup: 1, 2, 4, 8 or 16
  int ncol_chunks = 0;  // workgroups along the columns (gridDim.y)
  int nslabs = 0;       // gridDim.z
  int tiles_per_slab = 0;
  int64_t slab_begin[kKernelCrossMaxSlabs + 1] = {};
};
inline KernelSchedule kernel_product_schedule(int64_t nrows, int64_t nsum, int64_t ncols, int num_cus, int max_slabs) {
  KernelSchedule S;
  S.nrow_blocks = (int)((nrows + kKernelRows - 1) / kKernelRows);
  const int want = (int)((std::min<int64_t>(ncols, 16 * kKernelMaxColBlocks) + 15) / 16);
  S.col_blocks = 1;
  while (S.col_blocks < want) S.col_blocks *= 2;
  S.ncol_chunks = (int)((ncols + 16 * kKernelMaxColBlocks - 1) / (16 * kKernelMaxColBlocks));  // (ncols <= 256: one chunk, whatever col_blocks)
  const KernelSlabSplit s = kernel_slab_split((nsum + 15) / 16, (double)S.nrow_blocks * S.ncol_chunks, num_cus, max_slabs);
  S.nslabs = s.nslabs, S.tiles_per_slab = s.tiles_per_slab;
  kernel_slab_begin(s, nsum, S.slab_begin);
  return S;
}

// a run-time value to the instantiation compiled for it: f is called with a std::integral_constant. false: no such kernel (the
// caller reports it: there is no fallback). Every instantiation of a kernel is named by the ladder its launch goes down.
template <typename Fn> inline bool kernel_for_profile(int profile, Fn f) {
  switch (profile) {
    case KERNEL_RBF: return f(std::integral_constant<int, KERNEL_RBF>{});
    case KERNEL_MATERN12: return f(std::integral_constant<int, KERNEL_MATERN12>{});
    case KERNEL_MATERN32: return f(std::integral_constant<int, KERNEL_MATERN32>{});
    case KERNEL_MATERN52: return f(std::integral_constant<int, KERNEL_MATERN52>{});
    default: return false;
  }
}
template <typename Fn> inline bool kernel_for_ncb(int col_blocks, Fn f) {
  switch (col_blocks) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    case 16: return f(std::integral_constant<int, 16>{});
    default: return false;
  }
}
// dq = dpad / 4 coordinate quads: a kernel for d <= 16 and one for d <= kKernelMaxDim
template <typename Fn> inline bool kernel_for_dq(int dq, Fn f) {
  if (dq <= 4) return f(std::integral_constant<int, 4>{});
  return f(std::integral_constant<int, 16>{});
}

#ifdef __HIPCC__
// ---- device -------------------------------------------------------------------------------------------------------------
typedef double kd4_t __attribute__((ext_vector_type(4)));
typedef float kf4_t __attribute__((ext_vector_type(4)));
template <typename F> struct KernelAcc;
template <> struct KernelAcc<double> { using type = kd4_t; };
template <> struct KernelAcc<float> { using type = kf4_t; };
__device__ __forceinline__ kd4_t kernel_mfma(double a, double b, kd4_t c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
__device__ __forceinline__ kf4_t kernel_mfma(float a, float b, kf4_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// phi and chi = -2 dphi/dr2 of one r2 from one exp. matern12: chi = exp(-r) / r is DEFINED 0 at r2 = 0 (the diagonal, duplicate
// points, a clamped r2): chi D^2 tends to 0 there and must not become inf * 0.
template <typename F, int PROFILE> __device__ __forceinline__ void kernel_profile_pair(F r2, F &phi, F &chi) {
  if constexpr (PROFILE == KERNEL_RBF) {
    phi = chi = exp((F)-0.5 * r2);
  } else if constexpr (PROFILE == KERNEL_MATERN12) {
    const F r = sqrt(r2);
    phi = exp(-r);
    chi = r2 > (F)0 ? phi / r : (F)0;
  } else if constexpr (PROFILE == KERNEL_MATERN32) {
    const F a = (F)1.7320508075688772935 * sqrt(r2), p = (F)1 + a, e = exp(-a);
    phi = p * e;
    chi = (F)3 * e;
  } else {
    const F a = (F)2.2360679774997896964 * sqrt(r2), p = (F)1 + a, q = fma((F)(5.0 / 3.0), r2, p), e = exp(-a);
    phi = q * e;
    chi = (F)(5.0 / 3.0) * p * e;
  }
}
// phi alone (the unused chi folds away: the same expression in the same type)
template <typename F, int PROFILE> __device__ __forceinline__ F kernel_profile(F r2) {
#ifdef SLQ_KERNEL_PHI_ONE  // a measurement build (scripts/bench_kernelop.py): phi == 1, what the product costs without the profile
  return r2 < (F)0 ? r2 : (F)1;
#endif
  F phi, chi;
  kernel_profile_pair<F, PROFILE>(r2, phi, chi);
  return phi;
}

// One wave's 16 row points I against a tile J of 16 summed points:
//   G^T = z_J z_I^T   DQ MFMAs at most (d padded to 4 dq): A operand z_J from LDS (k-major: 16 consecutive words per k), B
//                     operand z_I from registers (loaded once). The result layout puts K^T[j][i = lane & 15] in the lane that
//                     must supply K[i = lane & 15][j] as the A operand of a second product: no shuffle, no LDS round trip;
//   r2                fma(-2, G^T, |z_i|^2 + |z_j|^2), clamped at 0; with the diagonal rule, 0 where j IS i.
// Fragment layouts (cdna_hip_programming.md §3): A[m = l & 15][k = l >> 4], B[k = l >> 4][n = l & 15]; C rows (l >> 4) + 4 reg
// in fp64, 4 (l >> 4) + reg in fp32 - jr(reg), the summed point within the tile that element reg of the lane belongs to.
// The next tile's z and norms travel in registers while this tile computes, and reach LDS between the two barriers of
// kernel_tile_walk (stash). Row points beyond rpad enter as zeros; the z of both sets are zero beyond their counts.
template <typename F, int DQ> struct KernelTile {
  using V4 = typename KernelAcc<F>::type;
  static constexpr bool F64 = sizeof(F) == 8;
  static constexpr int NT = 64 * kKernelWaves;
  static constexpr int ZPT = (DQ * 4 * 16 + NT - 1) / NT;  // z elements per thread and tile
  // what a kernel declares __shared__: F Zs[DQ * 4][16] (aligned 16), F Ns[16]; and keeps in registers: F zi[DQ], ni, zreg[ZPT], nreg

  // the wave's row points i0 .. i0 + 15: z_I^T as the B operand of the first product, |z_i|^2 for the lane's column i = lr
  __device__ __forceinline__ static void rows(const F *rzt, const F *rnrm, int rpad, int dq, int i0, int lr, int lk, F (&zi)[DQ], F &ni) {
    const bool i_ok = i0 + lr < rpad;
#pragma unroll
    for (int q = 0; q < DQ; ++q) zi[q] = (q < dq && i_ok) ? rzt[(int64_t)(4 * q + lk) * rpad + i0 + lr] : (F)0;
    ni = i_ok ? rnrm[i0 + lr] : (F)0;
  }
  // (the fetch of the next z tile - zreg[u] = element tid + u NT of the dq x 16 tile, nreg = the norm of point tid - is written out in
  // the fetch lambda of each kernel: as a function here it is the same loads, but the compiler then allocates registers differently
  // in most instantiations and three of them lose a resident workgroup; profiles/kerneltile_resources.txt)
  __device__ __forceinline__ static void stash(F (&Zs)[DQ * 4][16], F (&Ns)[16], int tid, const F (&zreg)[ZPT], F nreg) {
#pragma unroll
    for (int u = 0; u < ZPT; ++u) {
      const int e = tid + u * NT;
      if (e < DQ * 64) Zs[e >> 4][e & 15] = zreg[u];
    }
    if (tid < 16) Ns[tid] = nreg;
  }
  __device__ __forceinline__ static V4 gram(const F (&Zs)[DQ * 4][16], const F (&zi)[DQ], int dq, int lr, int lk) {
    V4 g = (V4)(F)0;
#pragma unroll
    for (int q = 0; q < DQ; ++q)
      if (q < dq) g = kernel_mfma(Zs[4 * q + lk][lr], zi[q], g);
    return g;
  }
  __device__ __forceinline__ static int jr(int lk, int r) { return F64 ? lk + 4 * r : 4 * lk + r; }
  // element r of the lane; diagonal: the summed point IS the row point, and the rule applies
  __device__ __forceinline__ static F r2(const V4 &g, int r, F ni, const F (&Ns)[16], int lk, bool diagonal) {
    F v = fma((F)-2, g[r], ni + Ns[jr(lk, r)]);
    v = fmax(v, (F)0);
    if (diagonal) v = (F)0;
    return v;
  }
};

// The tiles [t_begin, t_end) of a slab: fetch(t + 1) is in flight in registers while body(t) computes on what stash() put into
// LDS; two barriers per tile - every wave has read tile t, every wave sees tile t + 1.
template <typename Fetch, typename Stash, typename Body>
__device__ __forceinline__ void kernel_tile_walk(int t_begin, int t_end, const Fetch &fetch, const Stash &stash, const Body &body) {
  if (t_begin < t_end) {
    fetch(t_begin);
    stash();
  }
  __syncthreads();
  for (int t = t_begin; t < t_end; ++t) {
    const bool more = t + 1 < t_end;  // (uniform over the workgroup)
    if (more) fetch(t + 1);
    body(t);
    __syncthreads();
    if (more) stash();
    __syncthreads();
  }
}

// Y = s phi(r2) W. Grid (row blocks, column chunks, slabs); a wave owns 16 rows I and NCB 16-column tiles of the columns
// [col0, col0 + 16 NCB). Per tile J of 16 summed points: G^T and r2 of KernelTile; K = phi(r2), 4 values per lane, once per
// (i, j), whatever NCB is; acc += K W_J, 4 NCB MFMAs, W_J (16 x 16 NCB) from LDS, staged once per workgroup. Rows i >= nrows
// are computed on zero padding and never stored; points j >= nsum enter with W = 0 (phi is finite at the zero padding of z);
// columns g >= ncols likewise. s (and sigma2) come from params (device memory: a captured graph sees a hyperparameter change).
// gridDim.z > 1: slab z of the raw partial products at out + z * slab_stride. The order of j is fixed and nothing is atomic:
// identical calls give identical bits.
// A Layout says what differs between the operator's product and a cross product:
//   w_row<F, NC>(e), w_col<F, NC>(e)   element e of the 16 x NC tile of W -> (row, column): which thread fetches what, tuned
//                                      to the global access pattern and to the LDS banks of that layout
//   w_off(j, g), out_off(i, g)         where element (j, g) of W and (i, g) of the output live
//   chunk_cols<NC>()                   columns from one workgroup along gridDim.y to the next: NC or 256, the same number wherever
//                                      there is a second workgroup (each layout keeps the constant its kernel was compiled with)
//   kDiagonal                          r2 = 0 where the summed point IS the row point (one point set), or no such rule (two sets)
//   finish(sig, W, off, v)             the epilogue on v = s * acc; kNoise: sig = sigma2 in slab 0, else no sigma2 is read
//   kScaled, scale<F>()                a diagonal scale c of the (one) point set: Y = s diag(c) phi(r2) diag(c) W. c_j of
//                                      the summed points travels with |z_j|^2 - one word per point, fetched into a register, stashed to
//                                      Cs[16] between the two barriers - and multiplies the lane's four K values after the profile, once per
//                                      tile whatever NCB is; c_i meets s in the epilogue. Padding points carry c = 0. The branch is
//                                      compile-time: a layout with kScaled == false compiles to what it compiled to without it.
// (the LDS words of a scaled layout's c tile: a function, so that an unscaled instantiation does not hold them)
template <typename F> __device__ __forceinline__ F *kernel_scale_tile() {
  __shared__ F Cs[16];
  return Cs;
}
template <typename F, int PROFILE, int NCB, int DQ, typename Layout>
__device__ __forceinline__ void kernel_product(int nrows, int rpad, int nsum, int spad, int dq, const F *rzt, const F *rnrm, const F *szt, const F *snrm,
                                               const F *params, const F *W, int ncols, int tiles_per_slab, F *out, int64_t slab_stride, const Layout L) {
  using T = KernelTile<F, DQ>;
  using V4 = typename T::V4;
  constexpr bool F64 = T::F64;
  constexpr int NC = 16 * NCB;
  constexpr int WS = NC + (F64 ? (NC % 32 == 16 ? 0 : 16) : 4);  // row stride of the W tile: the 4 rows a read touches on distinct banks
  constexpr int NT = T::NT;
  constexpr int WPT = (16 * NC + NT - 1) / NT;  // W elements per thread and tile
  __shared__ __attribute__((aligned(16))) F Ws[16][WS];
  __shared__ __attribute__((aligned(16))) F Zs[DQ * 4][16];
  __shared__ F Ns[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int col0 = blockIdx.y * Layout::template chunk_cols<NC>();
  const int i0 = blockIdx.x * kKernelRows + wave * 16;
  int t_begin, t_end;
  kernel_slab_tiles<int>(spad >> 4, tiles_per_slab, (int)blockIdx.z, &t_begin, &t_end);

  F zi[DQ], ni;
  T::rows(rzt, rnrm, rpad, dq, i0, lr, lk, zi, ni);
  V4 acc[NCB];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) acc[cb] = (V4)(F)0;

  F wreg[WPT], zreg[T::ZPT], nreg = (F)0;
  [[maybe_unused]] F creg = (F)0;
  [[maybe_unused]] F *Cs = nullptr;
  if constexpr (Layout::kScaled) Cs = kernel_scale_tile<F>();
  auto fetch = [&](int t) {
    const int j0 = t * 16;
#pragma unroll
    for (int u = 0; u < WPT; ++u) {
      const int e = tid + u * NT, c = Layout::template w_col<F, NC>(e), j = j0 + Layout::template w_row<F, NC>(e);
      const int g = col0 + c;
      F v = (F)0;
      if (e < 16 * NC && j < nsum && g < ncols) v = W[L.w_off(j, g)];
      wreg[u] = v;
    }
#pragma unroll
    for (int u = 0; u < T::ZPT; ++u) {
      const int e = tid + u * NT, k = e >> 4, jj = e & 15;
      zreg[u] = (e < DQ * 64 && k < 4 * dq) ? szt[(int64_t)k * spad + j0 + jj] : (F)0;
    }
    if (tid < 16) nreg = snrm[j0 + tid];
    if constexpr (Layout::kScaled)
      if (tid < 16) creg = L.template scale<F>()[j0 + tid];  // (j0 + tid < spad: the scale has spad words, zeros beyond nsum)
  };
  auto stash = [&]() {
#pragma unroll
    for (int u = 0; u < WPT; ++u) {
      const int e = tid + u * NT;
      if (e < 16 * NC) Ws[Layout::template w_row<F, NC>(e)][Layout::template w_col<F, NC>(e)] = wreg[u];
    }
    T::stash(Zs, Ns, tid, zreg, nreg);
    if constexpr (Layout::kScaled)
      if (tid < 16) Cs[tid] = creg;
  };
  kernel_tile_walk(t_begin, t_end, fetch, stash, [&](int t) {
    const V4 g = T::gram(Zs, zi, dq, lr, lk);
    F kv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
      kv[r] = kernel_profile<F, PROFILE>(T::r2(g, r, ni, Ns, lk, Layout::kDiagonal && t * 16 + T::jr(lk, r) == i0 + lr));
    if constexpr (Layout::kScaled) {
#pragma unroll
      for (int r = 0; r < 4; ++r) kv[r] *= Cs[T::jr(lk, r)];
    }
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[cb] = kernel_mfma(kv[r], Ws[T::jr(lk, r)][cb * 16 + lr], acc[cb]);
  });
  const F s = params[0];
  F sig = (F)0;
  if constexpr (Layout::kNoise) sig = blockIdx.z == 0 ? params[1] : (F)0;
  F *o = out + (int64_t)blockIdx.z * slab_stride;
  [[maybe_unused]] F sc[4];  // s c_i of the lane's four rows
  if constexpr (Layout::kScaled) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + T::jr(lk, r);
      sc[r] = i < nrows ? s * L.template scale<F>()[i] : (F)0;
    }
  }
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) {
    const int g = col0 + cb * 16 + lr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + T::jr(lk, r);
      if (i < nrows && g < ncols) {
        const int64_t off = L.out_off(i, g);
        if constexpr (Layout::kScaled) o[off] = L.finish(sig, W, off, sc[r] * acc[cb][r]);
        else o[off] = L.finish(sig, W, off, s * acc[cb][r]);
      }
    }
  }
}
#endif  // __HIPCC__

}  // namespace slq
