// slq_radau.hpp — quadrature of a PREFIX of a Lanczos run, the Gauss-Radau rule and the per-stage statistics
// (slq_plan_quadrature_at, slq_quadrature_radau_batch).
//
// The Jacobi matrix J_m of the first m steps of a run is what a run of degree m produces, so the m-point Gauss rule of
// the prefix is the rule of that shorter run. With a lower bound a <= lambda_min(A) the (m + 1)-point Gauss-Radau rule
// with a prescribed node at a (Golub 1973; Golub & Meurant, Matrices, Moments and Quadrature, §6.2) is the Gauss rule
// of J_m bordered by
//   alpha_{m+1} = a + beta_m^2 / delta_m,   coupled to J_m by beta_m,
// where delta solves (J_m - a I) delta = beta_m^2 e_m by the forward recurrence
//   delta_1 = alpha_1 - a,   delta_j = alpha_j - a - beta_{j-1}^2 / delta_{j-1}
// (the pivots of the LDL^T factorisation of J_m - a I: all positive iff a lies below the smallest Ritz value). For f
// whose derivatives keep one sign (log, inverse, exp(-t x), powers) the Radau and the Gauss values bracket v^T f(A) v.
// Both rules go through the one first-row QL (ql_first_row_sorted, slq_kernels.hpp).
//   k_quadrature_at   one lane per probe: Gauss rule of J_m, then (rule 1) the bordered matrix and its rule
//   k_stage_reduce    {sum quad, sum quad^2, sum |quad - gauss|, count} over the probes: fixed slices, folded by a
//                     fixed tree - no float atomics, identical runs give identical bits
#pragma once

#include "slq_kernels.hpp"

namespace slq {

constexpr int kStageThreads = 256;

// m: size of the prefix (alpha rows 0 .. m-1, nu rows 1 .. m; the row stride stays st.bpad and the arrays have
// st.deg + 1 rows). LDS: 3 * (m + 1) * lanes doubles. rule 0: quad = Gauss value, nodes / weights P x m. rule 1: quad =
// Radau value, nodes / weights P x (m + 1); gauss (P doubles) receives the Gauss value in both cases.
// A probe that stopped at or before step m (its beta_m is zero or below residual_tol: the run took it as converged)
// has an exact Gauss rule; its Radau value IS its Gauss value, returned as the Gauss rule behind a zero-weight node at
// the endpoint. flags[0]: QL non-convergence, flags[1]: a pivot delta_j <= 0 (endpoint not below that probe's Ritz values).
__global__ __launch_bounds__(64) void k_quadrature_at(StepState st, int m, int rule, double endpoint, double residual_tol,
                                                      int lanes, int fun_id, double p0, double p1, double *__restrict__ quad,
                                                      double *__restrict__ gauss, double *__restrict__ nodes,
                                                      double *__restrict__ weights, int *__restrict__ flags) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int col = blockIdx.x * lanes + lane;
  if (lane >= lanes || col >= st.nprobes) return;
  const int kk = m + 1;  // rows of the LDS columns
  double *d = lds + lane, *e = lds + kk * lanes + lane, *z = lds + 2 * kk * lanes + lane;
#define D(i) d[(i) * lanes]
#define E(i) e[(i) * lanes]
#define Z(i) z[(i) * lanes]
  for (int i = 0; i < m; ++i) {
    D(i) = st.alpha[(int64_t)i * st.bpad + col];
    E(i) = (i + 1 < m) ? st.nu[(int64_t)(i + 1) * st.bpad + col] : 0.0;
    Z(i) = (i == 0) ? 1.0 : 0.0;
  }
  int bad = ql_first_row_sorted(d, e, z, m, lanes);
  const double vn2 = st.vnorm2[col];
  const int kout = rule ? kk : m;
  double s = 0.0;
  for (int i = 0; i < m; ++i) {
    const double th = D(i), tau = Z(i) * Z(i);
    // (rule 1: behind the slot of the zero-weight endpoint; overwritten below unless the probe stopped early)
    if (nodes) nodes[(int64_t)col * kout + (rule ? i + 1 : i)] = th;
    if (weights) weights[(int64_t)col * kout + (rule ? i + 1 : i)] = tau;
    if (fun_id >= 0) s += apply_fun(fun_id, p0, p1, th) * tau;
  }
  // an all-zero probe is 0/0 in the reference (lanczos.h:120): surface it as NaN
  const double gval = (vn2 > 0.0) ? s * vn2 : __builtin_nan("");
  if (gauss) gauss[col] = gval;
  double qval = gval;
  if (rule) {
    const double bm = st.nu[(int64_t)m * st.bpad + col];
    // (a Lanczos beta is a norm; a stand-alone batch may hand in a negative coupling, whose sign the rule does not see)
    const bool early = st.steps[col] < m || !(fabs(bm) >= residual_tol) || bm == 0.0;
    if (early) {
      if (nodes) nodes[(int64_t)col * kout] = endpoint;
      if (weights) weights[(int64_t)col * kout] = 0.0;
    } else {
      // J_m again (the QL consumed it), the pivots of J_m - a I, the border
      double delta = 0.0;
      bool neg = false;
      for (int i = 0; i < m; ++i) {
        const double a_i = st.alpha[(int64_t)i * st.bpad + col];
        const double b_i = (i > 0) ? st.nu[(int64_t)i * st.bpad + col] : 0.0;
        delta = (i == 0) ? a_i - endpoint : a_i - endpoint - (b_i * b_i) / delta;
        if (!(delta > 0.0)) neg = true;
        D(i) = a_i;
        E(i) = st.nu[(int64_t)(i + 1) * st.bpad + col];  // (i = m - 1: beta_m couples the border)
        Z(i) = (i == 0) ? 1.0 : 0.0;
      }
      D(m) = endpoint + (bm * bm) / delta;
      E(m) = 0.0;
      Z(m) = 0.0;
      if (neg) {
        atomicOr(flags + 1, 1);
      } else {
        bad |= ql_first_row_sorted(d, e, z, kk, lanes);
        double r = 0.0;
        for (int i = 0; i < kk; ++i) {
          const double th = D(i), tau = Z(i) * Z(i);
          if (nodes) nodes[(int64_t)col * kk + i] = th;
          if (weights) weights[(int64_t)col * kk + i] = tau;
          if (fun_id >= 0) r += apply_fun(fun_id, p0, p1, th) * tau;
        }
        qval = (vn2 > 0.0) ? r * vn2 : __builtin_nan("");
      }
    }
  }
  if (quad) quad[col] = qval;
  if (bad) atomicOr(flags, 1);
#undef D
#undef E
#undef Z
}

// out[0..3] = {sum_i quad_i, sum_i quad_i^2, sum_i |quad_i - gauss_i| (0 without gauss), P}. One workgroup: thread t
// adds the probes of its contiguous slice in order, the slices are folded pairwise in LDS (stride 128, 64, ... 1).
__global__ __launch_bounds__(kStageThreads) void k_stage_reduce(int P, const double *__restrict__ quad, const double *__restrict__ gauss,
                                                                double *__restrict__ out) {
  __shared__ double red[3][kStageThreads];
  const int t = threadIdx.x;
  const int i0 = (int)((int64_t)P * t / kStageThreads), i1 = (int)((int64_t)P * (t + 1) / kStageThreads);
  double s = 0.0, s2 = 0.0, w = 0.0;
  for (int i = i0; i < i1; ++i) {
    const double q = quad[i];
    s += q;
    s2 += q * q;
    if (gauss) w += fabs(q - gauss[i]);
  }
  red[0][t] = s;
  red[1][t] = s2;
  red[2][t] = w;
  __syncthreads();
  for (int h = kStageThreads / 2; h > 0; h >>= 1) {
    if (t < h) {
      red[0][t] += red[0][t + h];
      red[1][t] += red[1][t + h];
      red[2][t] += red[2][t + h];
    }
    __syncthreads();
  }
  if (t < 4) out[t] = t < 3 ? red[t][0] : (double)P;
}

// beta_m of a stand-alone batch into row deg of nu (k_load_tridiag leaves it zero), steps = deg: no early stop
__global__ void k_load_residual(StepState st, const double *__restrict__ beta_m, int nb) {
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= st.bpad) return;
  st.nu[(int64_t)st.deg * st.bpad + col] = col < nb ? beta_m[col] : 0.0;
  st.steps[col] = st.deg;
}

}  // namespace slq
