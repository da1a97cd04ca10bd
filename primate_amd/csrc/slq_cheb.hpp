// slq_cheb.hpp — Chebyshev moments (the kernel polynomial method): the kernels of slq_plan_run_chebyshev,
// slq_plan_moment_sum and slq_density_update_moments.
//
// With A~ = (A - c) / h and w_0 = v, w_1 = A~ v, w_{j+1} = 2 A~ w_j - w_{j-1} (w_j = T_j(A~) v), the moments
// mu_k = v^T T_k(A~) v follow from two sums per step (T_m T_n = (T_{m+n} + T_{|m-n|}) / 2):
//   mu_{2j+2} = 2 ||w_{j+1}||^2 - mu_0,        mu_{2j+1} = 2 w_{j+1}.w_j - mu_1.
// Step j is the orth-0 update pass w = sc A W_c - cB W_c - cp W_p with constant coefficients (step 0: sc = 1/h, cB = c/h,
// W_p unread; later sc = 2/h, cB = 2c/h, cp = 1), which stores w over W_p and reduces ||w||^2 and w.W_c already
// (k_csr_pass / k_csr_ring_pass / k_ring_pass with xt bit 0). Plans that take the sweeps run their product kernel and then
// k_cheb_axpy (k_cheb_3term after an unfused product). No float atomics; every sum in a fixed order.
// The action Y = sum_k c_k w_k (slq_plan_chebyshev_action) adds k_cheb_accumulate, launched between the steps
// of the same run while the w_k are still in the ring.
#pragma once

#include "slq_kernels.hpp"
#include "slq_action.hpp"   // (acc_fma: k_cheb_accumulate adds its columns as k_action_accumulate does)
#include "slq_density.hpp"  // (kDensEvalThreads: k_cheb_density_eval fills the scratch k_density_fold folds)

namespace slq {

// sum_partials with the rounding of every addition carried along (two-sum: the error term of each add is exact and summed
// beside the running sum), so that the result is the partials' sum rounded once. The moments are differences 2 s - mu_0 of sums
// over all blocks, and mu_0 is one itself: what the plain fixed-order sum loses over a few hundred blocks - a few ulp of mu_0 -
// is the whole rounding budget (k + 1) eps mu_0 of the first moments. Same fixed order as sum_partials: bitwise reproducible.
__device__ __forceinline__ void two_sum_acc(double &sum, double &err, double x) {
  const double t = sum + x;
  const double bb = t - sum;
  err += (sum - (t - bb)) + (x - bb);
  sum = t;
}
__device__ __forceinline__ double sum_partials_exact(const double *__restrict__ part, int nblk, int bpad, int col,
                                                     double *red /* 2 * kFinThreads doubles */) {
  const int c = threadIdx.x & 63, s = threadIdx.x >> 6;
  double a = 0.0, e = 0.0;
  if (col < bpad)
    for (int b = s; b < nblk; b += kFinSlices) two_sum_acc(a, e, part[(int64_t)b * bpad + col]);
  red[s * 64 + c] = a;
  red[kFinThreads + s * 64 + c] = e;
  __syncthreads();
  double tot = 0.0, te = 0.0;
#pragma unroll
  for (int k = 0; k < kFinSlices; ++k) {
    two_sum_acc(tot, te, red[k * 64 + c]);
    te += red[kFinThreads + k * 64 + c];
  }
  __syncthreads();
  return tot + te;
}

// After the update pass of step j (j = -1: before step 0, the partials are those of the probes' norm sweep): the step's two moments, the `outside` flags and the
// coefficients of the next step. mu: [2 deg + 1][bpad]. ratio: sphere probes are sqrt(n) g / ||g|| while the panel holds g
// (k_fin_init), and the moments are quadratic in the probe.
__global__ __launch_bounds__(kFinThreads) void k_fin_cheb(StepState st, const double *__restrict__ part, int nblk, int j,
                                                          double *__restrict__ mu, int *__restrict__ outside, double inv_h,
                                                          double c_over_h, double tol, int sphere) {
  __shared__ double red4[2 * kFinThreads];
  const int col = blockIdx.x * 64 + (threadIdx.x & 63);
  const int bp = st.bpad;
  double x = 0.0;
  const double s = sum_partials_exact(part, nblk, bp, col, red4);
  if (j >= 0) x = sum_partials_exact(part + (int64_t)nblk * bp, nblk, bp, col, red4);
  if ((threadIdx.x >> 6) != 0 || col >= bp) return;
  const int act = st.active[col];
  if (j < 0) {
    // mu_0 = ||v||^2 from the norm sweep's partials (sphere probes: n, as k_fin_init set it)
    mu[col] = act ? (sphere ? st.vnorm2[col] : s) : 0.0;
    outside[col] = 0;
    st.coefA[col] = act ? inv_h : 0.0;  // (padding columns and zero probes: zero coefficients, zero moments)
    st.coefA[bp + col] = 0.0;
    st.coefB[col] = act ? c_over_h : 0.0;
    return;
  }
  const double nu0 = st.nu[col];
  const double ratio = (sphere && act) ? st.vnorm2[col] / (nu0 * nu0) : 1.0;
  const double mu0 = mu[col];
  const double odd = j == 0 ? ratio * x : 2.0 * (ratio * x) - mu[bp + col];
  const double even = 2.0 * (ratio * s) - mu0;
  mu[(int64_t)(2 * j + 1) * bp + col] = odd;
  mu[(int64_t)(2 * j + 2) * bp + col] = even;
  // (written so that a NaN or an infinity raises the flag as well)
  const double bar = (1.0 + tol) * mu0;
  if (!(fabs(odd) <= bar) || !(fabs(even) <= bar)) outside[col] = 1;
  if (j == 0) {
    st.coefA[col] = act ? 2.0 * inv_h : 0.0;
    st.coefA[bp + col] = act ? 1.0 : 0.0;
    st.coefB[col] = act ? 2.0 * c_over_h : 0.0;
  }
}

// Sweeps, after a product kernel has left W = sc A W_c - cp W_p: w = W - cB W_c stored in place, ||w||^2 into slab 0 of the
// partials and w.W_c into slab 1 - k_axpy_norm with the cross term, one read-modify-write sweep.
template <typename F, int LPR>
__global__ __launch_bounds__(kBlock) void k_cheb_axpy(int n, F *W, const F *Wc, const double *__restrict__ coefB,
                                                      double *__restrict__ part, int bpad) {
  using VF = typename VecT<F>::type;
  constexpr int V = Geo<F, LPR>::V, PW = Geo<F, LPR>::PW, RPW = Geo<F, LPR>::RPW;
  __shared__ double red[kWaves * 64 * V];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / LPR, cl = lane % LPR;
  const int panel = blockIdx.y;
  const int64_t poff = (int64_t)panel * n * PW + cl * V;
  const int colbase = panel * PW + cl * V;
  VF cb;
#pragma unroll
  for (int v = 0; v < V; ++v) cb[v] = (F)coefB[colbase + v];
  VF nacc = (VF)(F)0, xacc = (VF)(F)0;
  const int stride = gridDim.x * kWaves * RPW;
  for (int row = (blockIdx.x * kWaves + wave) * RPW + g; row < n; row += stride) {
    const int64_t ro = poff + (int64_t)row * PW;
    const VF xc = *(const VF *)(Wc + ro);
    VF w = *(const VF *)(W + ro);
    w -= cb * xc;
    *(VF *)(W + ro) = w;
    nacc += w * w;
    xacc += w * xc;
  }
  block_reduce_columns<F, LPR>(nacc, red, part + (int64_t)blockIdx.x * bpad + panel * PW);
  block_reduce_columns<F, LPR>(xacc, red, part + ((int64_t)gridDim.x + blockIdx.x) * bpad + panel * PW);
}

// Unfused operators (host callback, device callback, Gram, the VALU dense kernel), in: T = A W_c unscaled.
// w = sc T - cp W_p - cB W_c, stored to Wn, with both sums: what k_3term + k_axpy_norm take two sweeps for.
template <typename F, int LPR>
__global__ __launch_bounds__(kBlock) void k_cheb_3term(int n, const F *T, const F *Wc, const F *Wp, F *Wn,
                                                       const double *__restrict__ coefA, const double *__restrict__ coefB,
                                                       double *__restrict__ part, int bpad, int first) {
  using VF = typename VecT<F>::type;
  constexpr int V = Geo<F, LPR>::V, PW = Geo<F, LPR>::PW, RPW = Geo<F, LPR>::RPW;
  __shared__ double red[kWaves * 64 * V];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / LPR, cl = lane % LPR;
  const int panel = blockIdx.y;
  const int64_t poff = (int64_t)panel * n * PW + cl * V;
  const int colbase = panel * PW + cl * V;
  VF sc, cp, cb;
#pragma unroll
  for (int v = 0; v < V; ++v) {
    sc[v] = (F)coefA[colbase + v];
    cp[v] = (F)coefA[bpad + colbase + v];
    cb[v] = (F)coefB[colbase + v];
  }
  VF nacc = (VF)(F)0, xacc = (VF)(F)0;
  const int stride = gridDim.x * kWaves * RPW;
  for (int row = (blockIdx.x * kWaves + wave) * RPW + g; row < n; row += stride) {
    const int64_t ro = poff + (int64_t)row * PW;
    const VF xc = *(const VF *)(Wc + ro);
    VF w = sc * *(const VF *)(T + ro);
    if (!first) w -= cp * *(const VF *)(Wp + ro);
    w -= cb * xc;
    *(VF *)(Wn + ro) = w;
    nacc += w * w;
    xacc += w * xc;
  }
  block_reduce_columns<F, LPR>(nacc, red, part + (int64_t)blockIdx.x * bpad + panel * PW);
  block_reduce_columns<F, LPR>(xacc, red, part + ((int64_t)gridDim.x + blockIdx.x) * bpad + panel * PW);
}

// a wave-uniform value into scalar registers (fp32: the conversion from the double leaves it in a vector register)
__device__ __forceinline__ float wave_uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ double wave_uniform(double v) { return lane_bcast(v, 0) /* (no lane is off in the prologue) */; }
// acc_fma with the coefficient as a SCALAR operand. fp32: left to itself the compiler pairs the four fmas of a column into
// two v_pk_fma_f32, which want the coefficient duplicated into a VGPR pair per column - 140 VGPRs at 16 columns, one resident
// workgroup per CU; v_fma_f32 is the instruction __builtin_fmaf compiles to, so the bits are the same.
__device__ __forceinline__ float acc_fma_scalar(float c, float x, float y) {
  asm("v_fma_f32 %0, %1, %2, %0" : "+v"(y) : "s"(c), "v"(x));
  return y;
}
__device__ __forceinline__ double acc_fma_scalar(double c, double x, double y) { return acc_fma(c, x, y); }

// Y[row, :] (+)= sum_{i < nc} c_{t0+i} W_{t0+i}[row, :] for nc <= kChebAccCols finished ring columns (w_t in slot t mod S), t
// ascending, one fma per column: the same bits whatever the grid. k_action_accumulate with ONE polynomial for every probe:
// coef: the [nsteps + 1] coefficients as doubles, read at wave-uniform indices - scalar loads, scalar registers - and rounded
//   to F once here; no lane holds a coefficient (k_action_accumulate: 8 x V VGPRs of them), which is what admits 16 columns;
// live: bit i set iff column t0 + i is read - computed on the host (c_{t0+i} != 0.0, or every bit under SLQ_ACC_SKIP=0): a
//   column whose bit is off is not read (0 * x adds nothing for finite x: bitwise neutral). Bits i >= nc are never set;
// init != 0: Y is written, not read (the first launch of a run).
// Every live column load of a row group is issued before the first fma; one row group per wave and iteration.
template <typename F, int LPR>
__global__ __launch_bounds__(kBlock) void k_cheb_accumulate(int n, const F *__restrict__ ring, int64_t slot_stride, int S, int t0, int nc,
                                                            unsigned live, const double *__restrict__ coef, F *__restrict__ Y, int init) {
  using VF = typename VecT<F>::type;
  constexpr int V = Geo<F, LPR>::V, PW = Geo<F, LPR>::PW, RPW = Geo<F, LPR>::RPW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / LPR, cl = lane % LPR;
  // Addresses are a wave-uniform 64-bit base (column, panel, the workgroup's first row: scalar registers) plus ONE small
  // per-lane byte offset shared by every column - with a 64-bit address per column and lane the compiler keeps 16 of them
  // in vector registers (fp64, 64 lanes per row: 111 VGPRs against 76).
  const unsigned lrow = (unsigned)(wave * RPW + g);
  const unsigned vbyte = (lrow * PW + cl * V) * (unsigned)sizeof(F);  // < kWaves * 64 * V * sizeof(F) = 8 KiB
  const int64_t pbase = (int64_t)blockIdx.y * n * PW;
  live &= (1u << nc) - 1u;
  // (branch-free: a column past nc takes column t0 again and is never live - the prologue stays straight-line code)
  F c[kChebAccCols];
  const char *U[kChebAccCols];
#pragma unroll
  for (int i = 0; i < kChebAccCols; ++i) {
    const int t = t0 + (i < nc ? i : 0);
    c[i] = wave_uniform((F)coef[t]);
    U[i] = (const char *)(ring + (int64_t)ring_slot(t, S) * slot_stride + pbase);
  }
  char *Yp = (char *)(Y + pbase);
  const int stride = gridDim.x * kWaves * RPW;
#pragma unroll 1
  for (int rb = blockIdx.x * kWaves * RPW; rb < n; rb += stride) {  // (the workgroup's first row: wave-uniform)
    const int64_t ro = (int64_t)rb * PW * (int64_t)sizeof(F);
    if (rb + (int)lrow < n) {
      VF y = init ? (VF)(F)0 : stream_load<SLQ_SWEEP_LDW>((const VF *)(Yp + ro + vbyte));
      // every live column load of the row group is issued before the first use
      VF x[kChebAccCols];
#pragma unroll
      for (int i = 0; i < kChebAccCols; ++i)
        if ((live >> i) & 1u) x[i] = *(const VF *)(U[i] + ro + vbyte);
#pragma unroll
      for (int i = 0; i < kChebAccCols; ++i) {
        if ((live >> i) & 1u) {
#pragma unroll
          for (int v = 0; v < V; ++v) y[v] = acc_fma_scalar(c[i], x[i][v], y[v]);
        }
      }
      stream_store<SLQ_SWEEP_ST>((VF *)(Yp + ro + vbyte), y);
    }
  }
}

// quad[p] = sum_{k < ncoef} coef[k] mu[k][p], k ascending: one lane per probe.
__global__ __launch_bounds__(64) void k_moment_sum(int P, int bpad, int ncoef, const double *__restrict__ coef,
                                                   const double *__restrict__ mu, double *__restrict__ quad) {
  const int col = blockIdx.x * 64 + threadIdx.x;
  if (col >= P) return;
  double s = 0.0;
  for (int k = 0; k < ncoef; ++k) s += coef[k] * mu[(int64_t)k * bpad + col];
  quad[col] = s;
}

// The density of the kernel polynomial method on a grid: one lane per (probe, grid column) as in k_density_eval - block b covers
// probe b / nbg and columns (b % nbg) * 256 + [0, 256) of the same P x (G + 2) scratch. The probe's damped moments g_k mu_k
// (doubled for k >= 1) pass through LDS in chunks of kChebChunk; T_k(x~) runs by the forward recurrence, k ascending, carried
// across the chunks in registers. damp null: g_k = 1. The two `outside` columns are 0: a grid point outside the interval is
// refused on the host.
constexpr int kChebChunk = 256;
__global__ __launch_bounds__(kDensEvalThreads) void k_cheb_density_eval(int G, int K, int bpad, const double *__restrict__ mu,
                                                                        const double *__restrict__ damp,
                                                                        const double *__restrict__ grid, double center, double h,
                                                                        int nbg, double *__restrict__ phi) {
  static_assert(kChebChunk == kDensEvalThreads, "one moment per thread and chunk");
  __shared__ double gm[kChebChunk];
  const int p = blockIdx.x / nbg;
  const int g = (blockIdx.x % nbg) * kDensEvalThreads + threadIdx.x;
  const int G2 = G + 2;
  const bool point = g < G;
  const double x = point ? (grid[g] - center) / h : 0.0;
  double tp = 1.0, tc = x;  // T_{k-1}, T_k at the head of a chunk's k (k = 1 first)
  double s = 0.0;
  for (int k0 = 0; k0 < K; k0 += kChebChunk) {
    const int k = k0 + (int)threadIdx.x;
    if (k < K) gm[threadIdx.x] = (k == 0 ? 1.0 : 2.0) * (damp ? damp[k] : 1.0) * mu[(int64_t)k * bpad + p];
    __syncthreads();
    const int kn = min(kChebChunk, K - k0);
    if (point) {
      int i = 0;
      if (k0 == 0) {
        s = gm[0];
        i = 1;
      }
      for (; i < kn; ++i) {
        s += gm[i] * tc;
        const double tn = 2.0 * x * tc - tp;
        tp = tc;
        tc = tn;
      }
    }
    __syncthreads();
  }
  if (g < G2) phi[(int64_t)p * G2 + g] = point ? s / (M_PI * h * sqrt(1.0 - x * x)) : 0.0;
}

}  // namespace slq
