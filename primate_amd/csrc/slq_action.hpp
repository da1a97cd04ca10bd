// slq_action.hpp — the accumulation of two-pass f(A)v (recompute plans: slq_plan_create_recompute).
//
// Two-pass Lanczos (Borici 2000; Frommer & Simoncini 2008): pass 1 is the ordinary run on the small ring and yields T; the
// coefficients g_t = ||x|| (Y (f(theta) * Y[0,:]))_t / nu_t come out of T alone (k_fun_coeffs); pass 2 runs the same recurrence
// again from the same probes and adds g_t W_t into an output panel while W_t is still in the ring. A run's sums are taken in a
// fixed order, so pass 2 reproduces every W_t bit for bit.
//   k_action_accumulate   Y[row, :] (+)= sum_{i < nc} g_{t0+i}[:] * W_{t0+i}[row, :] for nc <= kAccCols finished ring columns,
//                         ascending t, one fma per column: the same bits whatever the grid
#pragma once

#include "slq_kernels.hpp"

namespace slq {

// (kAccCols - ring columns one accumulation launch consumes at most: slq_format.hpp)

__device__ __forceinline__ double acc_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float acc_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// coef: row t0 of the [deg][bpad] coefficients (doubles, rounded to F once here, as the kept-basis combiner rounds its own).
// init != 0: Y is written, not read (the first launch of a replay: no memset, one panel read less).
// skip_zero_cols: a column whose coefficient is zero for EVERY probe of the panel - probes past an early stop, trailing steps
// of a converged f - is not read (0 * x adds nothing for finite x: bitwise neutral; SLQ_ACC_SKIP=0 reads them all).
// Columns i >= nc are never live: one instantiation per (F, LPR) serves every nc, the guards are wave-uniform.
// cols_stat: null, or {columns read, columns offered} summed over launches and panels (slq_plan_action_columns).
// One row group per wave and iteration: with two (k_reorth_update's SLQ_UPD_UR) the 16 loads in flight cost 152 (fp64) / 184 (fp32)
// VGPRs - one resident workgroup per CU instead of two - and measured no faster.
template <typename F, int LPR>
__global__ __launch_bounds__(kBlock) void k_action_accumulate(int n, const F *__restrict__ ring, int64_t slot_stride, int S, int t0, int nc,
                                                              const double *__restrict__ coef, int bpad, F *__restrict__ Y, int init,
                                                              int skip_zero_cols, unsigned long long *__restrict__ cols_stat) {
  using VF = typename VecT<F>::type;
  constexpr int V = Geo<F, LPR>::V, PW = Geo<F, LPR>::PW, RPW = Geo<F, LPR>::RPW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / LPR, cl = lane % LPR;
  const int panel = blockIdx.y;
  const int64_t poff = (int64_t)panel * n * PW + cl * V;
  // a lane owns its V probe columns for the whole kernel: nc x V coefficients in registers
  VF gm[kAccCols];
  unsigned live = 0;
  const double *cp = coef + panel * PW + cl * V;
#pragma unroll
  for (int i = 0; i < kAccCols; ++i) {
    // (branch-free: a column past nc reads row 0 again and takes a zero - the prologue stays straight-line code)
    const int64_t row = (int64_t)(i < nc ? i : 0) * bpad;
    const F on = i < nc ? (F)1 : (F)0;
    bool nz = false;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      gm[i][v] = on * (F)cp[row + v];
      nz = nz || gm[i][v] != (F)0;
    }
    if (__builtin_amdgcn_ballot_w64(nz) != 0ull) live |= 1u << i;  // (the wave's lanes cover every probe of the panel)
  }
  if (!skip_zero_cols) live = ~0u;
  live &= (1u << nc) - 1u;  // (columns past nc are never live)
  live = __builtin_amdgcn_readfirstlane(live);
  if (cols_stat && blockIdx.x == 0 && threadIdx.x == 0) {
    atomicAdd(cols_stat, (unsigned long long)__builtin_popcount(live));
    atomicAdd(cols_stat + 1, (unsigned long long)nc);
  }
  const F *U[kAccCols];
#pragma unroll
  for (int i = 0; i < kAccCols; ++i) U[i] = ring + (int64_t)ring_slot(t0 + (i < nc ? i : 0), S) * slot_stride + poff;
  F *Yp = Y + poff;
  const int stride = gridDim.x * kWaves * RPW;
#pragma unroll 1
  for (int row = (blockIdx.x * kWaves + wave) * RPW + g; row < n; row += stride) {
    const int64_t ro = (int64_t)row * PW;
    VF y = init ? (VF)(F)0 : stream_load<SLQ_SWEEP_LDW>((const VF *)(Yp + ro));
    // every column load of the row group is issued before the first use
    VF x[kAccCols];
#pragma unroll
    for (int i = 0; i < kAccCols; ++i)
      if ((live >> i) & 1u) x[i] = *(const VF *)(U[i] + ro);
#pragma unroll
    for (int i = 0; i < kAccCols; ++i) {
      if ((live >> i) & 1u) {
#pragma unroll
        for (int v = 0; v < V; ++v) y[v] = acc_fma(gm[i][v], x[i][v], y[v]);
      }
    }
    stream_store<SLQ_SWEEP_ST>((VF *)(Yp + ro), y);
  }
}

}  // namespace slq
