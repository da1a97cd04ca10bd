// slq_density.hpp — spectral density of stochastic Lanczos quadrature on the device (slq_density_*).
//
// Every probe's Gauss rule (nodes theta_pk, weights tau_pk, sum_k tau_pk = 1: what k_quadrature leaves in a plan's
// nodes_d / weights_d) is a discrete form of the per-probe spectral measure
//   psi(x; A, v) = sum_i |u_i^T v|^2 delta(x - lambda_i)        (reference: src/primate/integrate.py:30-35)
// smoothed by a kernel K and sampled on a grid (Lin, Saad, Yang: Approximating spectral densities of large matrices,
// SIAM Review 2016):  phi_p(x_g) = ||v_p||^2 sum_k tau_pk K(x_g, theta_pk).
// Two passes, no float atomics, so two identical runs give bitwise identical statistics:
//   k_density_eval   one lane per (probe, grid column), the sum over k in node order -> a P x (G + 2) scratch;
//                    columns G and G + 1 hold the node mass below and above the grid
//   k_density_fold   per grid column, the batch mean and M2 over the P probes (fixed probe slices, folded in slice
//                    order), merged into the running (mean, M2) with the batch-Welford formula of
//                    primate_amd.estimators.Covariance.update
#pragma once

#include "slq_kernels.hpp"  // (apply_fun)

namespace slq {

enum { kDensGaussian = 0, kDensLorentzian = 1, kDensHistogram = 2, kDensCdf = 3 };
constexpr int kDensEvalThreads = 256;
constexpr int kDensFoldWaves = 16;

// Block b covers probe b / nbg and grid columns (b % nbg) * 256 + [0, 256). c0, c1: the kernel's constants
// (gaussian: 1 / (2 sigma^2), 1 / (sigma sqrt(2 pi)); lorentzian: sigma^2, sigma / pi; unused otherwise).
// grid: G points, or G + 1 bin edges for the histogram. Zero-weight nodes (the zero tail of an early stop) add 0.
__global__ __launch_bounds__(kDensEvalThreads) void k_density_eval(int kind, int G, int k, const double *__restrict__ nodes,
                                                                   const double *__restrict__ weights,
                                                                   const double *__restrict__ vnorm2,
                                                                   const double *__restrict__ grid, double c0, double c1,
                                                                   int nbg, double *__restrict__ phi) {
  const int p = blockIdx.x / nbg;
  const int g = (blockIdx.x % nbg) * kDensEvalThreads + threadIdx.x;
  const int G2 = G + 2;
  if (g >= G2) return;
  const double *th = nodes + (int64_t)p * k, *tau = weights + (int64_t)p * k;
  double s = 0.0;
  if (g < G) {
    const double x = grid[g];
    switch (kind) {
      case kDensGaussian:
        for (int i = 0; i < k; ++i) {
          const double d = x - th[i];
          s += tau[i] * exp(-(d * d) * c0);
        }
        s *= c1;
        break;
      case kDensLorentzian:
        for (int i = 0; i < k; ++i) {
          const double d = x - th[i];
          s += tau[i] / (d * d + c0);
        }
        s *= c1;
        break;
      case kDensHistogram: {
        const double hi = grid[g + 1];  // bin [x, hi)
        for (int i = 0; i < k; ++i) s += (th[i] >= x && th[i] < hi) ? tau[i] : 0.0;
        break;
      }
      default:  // cdf: mass strictly below x
        for (int i = 0; i < k; ++i) s += th[i] < x ? tau[i] : 0.0;
        break;
    }
  } else if (g == G) {  // below the grid: theta < x_0 (the first edge for the histogram)
    const double lo = grid[0];
    for (int i = 0; i < k; ++i) s += th[i] < lo ? tau[i] : 0.0;
  } else {  // above: theta > x_{G-1}, or theta >= the last edge (the bins are half-open)
    const bool hist = kind == kDensHistogram;
    const double hi = grid[hist ? G : G - 1];
    for (int i = 0; i < k; ++i) s += (hist ? th[i] >= hi : th[i] > hi) ? tau[i] : 0.0;
  }
  phi[(int64_t)p * G2 + g] = s * vnorm2[p];
}

// One lane per grid column (64 per block), 16 waves split the probes into fixed contiguous slices. na: probes folded
// before this batch. flags[0] collects QL non-convergence (the device word rule_fail, or host_fail when the host
// already knows it), flags[1] the ring bail-out word of the plan; both are read back by slq_density_get.
__global__ __launch_bounds__(64 * kDensFoldWaves) void k_density_fold(int P, int G2, int64_t na, const double *__restrict__ phi,
                                                                      double *__restrict__ mean, double *__restrict__ m2,
                                                                      const int *__restrict__ rule_fail, int host_fail,
                                                                      const int *__restrict__ ring_fail, int *__restrict__ flags) {
  __shared__ double red[kDensFoldWaves][64];
  __shared__ double mb_s[64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int g = blockIdx.x * 64 + lane;
  const bool live = g < G2;
  const int p0 = (int)((int64_t)P * w / kDensFoldWaves), p1 = (int)((int64_t)P * (w + 1) / kDensFoldWaves);
  double s = 0.0;
  if (live)
    for (int p = p0; p < p1; ++p) s += phi[(int64_t)p * G2 + g];
  red[w][lane] = s;
  __syncthreads();
  if (w == 0) {
    double t = 0.0;
    for (int i = 0; i < kDensFoldWaves; ++i) t += red[i][lane];
    mb_s[lane] = t / (double)P;
  }
  __syncthreads();
  const double mb = mb_s[lane];
  double q = 0.0;
  if (live)
    for (int p = p0; p < p1; ++p) {
      const double d = phi[(int64_t)p * G2 + g] - mb;
      q += d * d;
    }
  red[w][lane] = q;  // (every read of red's sums happened before the barrier above)
  __syncthreads();
  if (w == 0 && live) {
    double m2b = 0.0;
    for (int i = 0; i < kDensFoldWaves; ++i) m2b += red[i][lane];
    const double nb = (double)P, nn = (double)na + nb;
    const double ma = mean[g], delta = mb - ma;
    m2[g] = m2[g] + (m2b + ((double)na * nb / nn) * (delta * delta));
    mean[g] = ma + (nb / nn) * delta;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    flags[0] = flags[0] | host_fail | (rule_fail ? *rule_fail : 0);
    flags[1] = flags[1] | *ring_fail;
  }
}

// quad[p] = sum_k f(theta_pk) tau_pk ||v_p||^2 from a rule already on the device: the reduction of k_quadrature, in the
// same order and form, for a slq_plan_quadrature that follows a density update of the same run (one QL per run).
__global__ __launch_bounds__(64) void k_rule_reduce(int P, int k, const double *__restrict__ nodes, const double *__restrict__ weights,
                                                    const double *__restrict__ vnorm2, int fun_id, double p0, double p1,
                                                    double *__restrict__ quad) {
  const int col = blockIdx.x * 64 + threadIdx.x;
  if (col >= P) return;
  double s = 0.0;
  if (fun_id >= 0)
    for (int i = 0; i < k; ++i) s += apply_fun(fun_id, p0, p1, nodes[(int64_t)col * k + i]) * weights[(int64_t)col * k + i];
  const double vn2 = vnorm2[col];
  quad[col] = (vn2 > 0.0) ? s * vn2 : __builtin_nan("");
}

}  // namespace slq
