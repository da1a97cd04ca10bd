// slq_toeplitz.hpp — the Toeplitz operator as far as the host decides it. Plain C++ (no HIP include): the pass
// structure of a product as a value (ToeplitzPlan, toeplitz_plan: slq_debug_toeplitz_plan, slq_plan_shape.hpp), the validation of
// c and r, the radix-2 transform in double that computes the symbol, and the tables the device passes read (the symbol in the
// order the forward passes leave, the twiddles of every level) - all of them run without a device (scripts/toeplitz_check.cpp).
// The kernels are in slq_toeplitz.hip; slq.hip sees only toeplitz_prepare / toeplitz_launch below.
//
// A_ij = c[i-j] (i >= j), r[j-i] (j > i), n x n. L: the smallest power of two >= 2n. e = [c_0 .. c_{n-1}, 0 .. 0, r_{n-1} .. r_1]
// (L entries), s = FFT_L(e): A x = (IFFT_L(s . FFT_L([x, 0])))[0 .. n). The panel row (PW reals) is PW/2 complex numbers, so a
// complex transform along the rows transforms probes 2q and 2q+1 at once (A is real).
//
// L = L_1 L_2 .. L_m (m <= 3), position pos = p_1 (L_2 .. L_m) + p_2 (L_3 .. L_m) + .. + p_m. Forward level j (j < m): a
// decimation-in-frequency transform of length L_j over p_j, then the twiddle W_{L_j S_j}^{s bitrev(p_j)} with S_j = L_{j+1} .. L_m
// and s the position behind p_j. The last level transforms, multiplies by the symbol and transforms back in one kernel; the inverse
// levels multiply by the conjugate twiddle and run the decimation-in-time transform that consumes the permuted order. After the
// forward passes position pos holds frequency k(pos) = sum_j bitrev_{L_j}(p_j) L_1 .. L_{j-1}: the symbol is stored at pos, and
// nothing is permuted on the device.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

namespace slq {

constexpr int kToeplitzMaxLog2L = 23;                                      // L <= 2^23
constexpr int64_t kToeplitzMaxN = (int64_t)1 << (kToeplitzMaxLog2L - 1);   // n <= 2^22
constexpr int kToeplitzMaxSub = 1024;     // points of a transform a workgroup keeps in LDS (128 bytes each: 128 KiB)
constexpr int kToeplitzMinTile = 256;     // rows of an LDS tile at least (shorter transforms: several side by side)
constexpr int kToeplitzRowBytes = 128;    // contiguous bytes of every row access of a workgroup
constexpr int kToeplitzTab = 1024;        // W_1024^t, t < 512: the twiddles of the transforms inside LDS
constexpr int kToeplitzBlock = 256;

struct ToeplitzPlan {
  int64_t n = 0, L = 0;
  int log2L = 0;
  int levels = 0;            // 1: one kernel; 2: three kernels; 3: five
  int lg[3] = {0, 0, 0};     // log2 L_j
  int cg = 0;                // complex columns of a workgroup (128 bytes)
  int tile_rows[3] = {0, 0, 0};  // rows of the LDS tile of level j's kernel(s)
  size_t lds_bytes = 0;      // of the largest kernel (tile + twiddle table)
  size_t ws_bytes = 0;       // complex workspace, one panel in flight (0: one kernel)
  int launches = 0;          // per panel
};

inline int toeplitz_log2_ceil(int64_t v) {
  int l = 0;
  while (((int64_t)1 << l) < v) ++l;
  return l;
}

// esize: 4 or 8. pw: the panel width (reals per row), a power of two >= 16 (fp64) / 32 (fp32). n must be in [1, kToeplitzMaxN].
inline ToeplitzPlan toeplitz_plan(int64_t n, int esize, int pw) {
  ToeplitzPlan P;
  P.n = n;
  P.log2L = toeplitz_log2_ceil(2 * n);
  P.L = (int64_t)1 << P.log2L;
  P.cg = kToeplitzRowBytes / (2 * esize);
  const int sub = toeplitz_log2_ceil(kToeplitzMaxSub);
  const int l = P.log2L;
  if (l <= sub) {
    P.levels = 1, P.lg[0] = l;
  } else if (l <= 2 * sub) {
    P.levels = 2, P.lg[1] = (l + 1) / 2, P.lg[0] = l - P.lg[1];
  } else {
    P.levels = 3, P.lg[2] = (l + 2) / 3, P.lg[1] = (l - P.lg[2] + 1) / 2, P.lg[0] = l - P.lg[2] - P.lg[1];
  }
  const size_t row = (size_t)P.cg * 2 * esize;
  size_t rows_max = 0;
  for (int j = 0; j < P.levels; ++j) {
    int64_t rows = (int64_t)1 << P.lg[j];
    if (rows < kToeplitzMinTile) rows = kToeplitzMinTile;
    if (rows > P.L) rows = P.L;
    P.tile_rows[j] = (int)rows;
    if ((size_t)rows > rows_max) rows_max = (size_t)rows;
  }
  P.lds_bytes = rows_max * row + (size_t)(kToeplitzTab / 2) * 2 * esize;
  P.ws_bytes = P.levels > 1 ? (size_t)P.L * (size_t)pw * esize : 0;
  P.launches = 2 * P.levels - 1;
  return P;
}

inline int64_t toeplitz_bitrev(int64_t v, int bits) {
  int64_t r = 0;
  for (int b = 0; b < bits; ++b) r |= ((v >> b) & 1) << (bits - 1 - b);
  return r;
}
// the frequency position pos holds after the forward passes
inline int64_t toeplitz_freq_of(const ToeplitzPlan &P, int64_t pos) {
  int64_t k = 0, below = P.log2L;
  int shift = 0;
  for (int j = 0; j < P.levels; ++j) {
    below -= P.lg[j];
    const int64_t pj = (pos >> below) & (((int64_t)1 << P.lg[j]) - 1);
    k += toeplitz_bitrev(pj, P.lg[j]) << shift;
    shift += P.lg[j];
  }
  return k;
}

// exp(-2 pi i k / N) in double, from the octant of k (exact at the multiples of N/8 up to the rounding of sqrt 1/2)
inline std::complex<double> toeplitz_root(int64_t k, int64_t N) {
  k %= N;
  if (k < 0) k += N;
  if (8 * k % N == 0) {
    const double h = 0.70710678118654752440;
    const std::complex<double> oct[8] = {{1, 0}, {h, -h}, {0, -1}, {-h, -h}, {-1, 0}, {-h, h}, {0, 1}, {h, h}};
    return oct[8 * k / N];
  }
  const long double a = -2.0L * 3.14159265358979323846264338327950288L * (long double)k / (long double)N;
  return {(double)cosl(a), (double)sinl(a)};
}

// In place, natural order in and out: x <- FFT_L(x), L = 2^log2L (decimation in time on the bit-reversed input; the roots from one table of
// L/2 entries computed directly, not by recurrence). O(L log L), double.
inline void toeplitz_host_fft(std::vector<std::complex<double>> &x, int log2L) {
  const int64_t L = (int64_t)1 << log2L;
  for (int64_t i = 0; i < L; ++i) {
    const int64_t j = toeplitz_bitrev(i, log2L);
    if (j > i) std::swap(x[(size_t)i], x[(size_t)j]);
  }
  std::vector<std::complex<double>> w((size_t)(L > 1 ? L / 2 : 1));
  for (int64_t k = 0; k < L / 2; ++k) w[(size_t)k] = toeplitz_root(k, L);
  for (int s = 0; s < log2L; ++s) {
    const int64_t h = (int64_t)1 << s, step = L / (2 * h);
    for (int64_t b = 0; b < L; b += 2 * h)
      for (int64_t o = 0; o < h; ++o) {
        const std::complex<double> u = x[(size_t)(b + o)], t = x[(size_t)(b + o + h)] * w[(size_t)(o * step)];
        x[(size_t)(b + o)] = u + t, x[(size_t)(b + o + h)] = u - t;
      }
  }
}

// c and r (NULL: c) rounded to the dtype (esize 4: through float) into cr, rr; the first entry that is not finite in the dtype is
// named in msg (returns false). symmetric: the rounded r[1:] equals c[1:] bitwise.
inline bool toeplitz_round_values(int64_t n, int esize, const double *c, const double *r, std::vector<double> &cr, std::vector<double> &rr, bool *symmetric, char *msg,
                                  size_t nmsg) {
  cr.resize((size_t)n), rr.resize((size_t)n);
  auto rnd = [esize](double v) { return esize == 4 ? (double)(float)v : v; };
  for (int64_t i = 0; i < n; ++i) {
    cr[(size_t)i] = rnd(c[i]);
    if (!std::isfinite(cr[(size_t)i])) {
      snprintf(msg, nmsg, "Toeplitz operator: c[%lld] = %g is not finite in the operator's dtype", (long long)i, c[i]);
      return false;
    }
  }
  bool sym = true;
  for (int64_t i = 0; i < n; ++i) {
    rr[(size_t)i] = i == 0 ? cr[0] : rnd(r ? r[i] : c[i]);  // (r[0] is ignored)
    if (!std::isfinite(rr[(size_t)i])) {
      snprintf(msg, nmsg, "Toeplitz operator: r[%lld] = %g is not finite in the operator's dtype", (long long)i, r[i]);
      return false;
    }
    if (i > 0 && memcmp(&rr[(size_t)i], &cr[(size_t)i], 8) != 0) sym = false;
  }
  *symmetric = sym;
  return true;
}

// s = FFT_L(e) of the rounded values, natural order, double
inline std::vector<std::complex<double>> toeplitz_symbol(const ToeplitzPlan &P, const std::vector<double> &cr, const std::vector<double> &rr) {
  std::vector<std::complex<double>> e((size_t)P.L, std::complex<double>(0.0, 0.0));
  for (int64_t i = 0; i < P.n; ++i) e[(size_t)i] = cr[(size_t)i];
  for (int64_t i = 1; i < P.n; ++i) e[(size_t)(P.L - i)] = rr[(size_t)i];
  toeplitz_host_fft(e, P.log2L);
  return e;
}

// What the device holds, as words of the operator's dtype (interleaved re, im):
//   sym   L complex: s[k(pos)] / L at pos (the 1/L of the inverse transform is folded in: a power of two, exact)
//   tab   512 complex: W_1024^t
//   tw[j] (j < levels - 1) L_j S_j complex: W_{L_j S_j}^{s bitrev(p)} at p S_j + s
template <typename F> inline void toeplitz_pack(const std::complex<double> *v, size_t count, F *out) {
  for (size_t i = 0; i < count; ++i) out[2 * i] = (F)v[i].real(), out[2 * i + 1] = (F)v[i].imag();
}
template <typename F> inline void toeplitz_device_symbol(const ToeplitzPlan &P, const std::vector<std::complex<double>> &s, F *out) {
  const double inv = 1.0 / (double)P.L;
  for (int64_t pos = 0; pos < P.L; ++pos) {
    const std::complex<double> v = s[(size_t)toeplitz_freq_of(P, pos)] * inv;
    out[2 * pos] = (F)v.real(), out[2 * pos + 1] = (F)v.imag();
  }
}
template <typename F> inline void toeplitz_device_tab(F *out) {
  for (int t = 0; t < kToeplitzTab / 2; ++t) {
    const std::complex<double> w = toeplitz_root(t, kToeplitzTab);
    out[2 * t] = (F)w.real(), out[2 * t + 1] = (F)w.imag();
  }
}
inline int64_t toeplitz_level_stride_log2(const ToeplitzPlan &P, int j) {
  int s = 0;
  for (int i = j + 1; i < P.levels; ++i) s += P.lg[i];
  return s;
}
template <typename F> inline void toeplitz_device_twiddles(const ToeplitzPlan &P, int j, F *out) {
  const int ls = (int)toeplitz_level_stride_log2(P, j);
  const int64_t S = (int64_t)1 << ls, Lj = (int64_t)1 << P.lg[j], N = Lj * S;
  for (int64_t p = 0; p < Lj; ++p) {
    const int64_t k1 = toeplitz_bitrev(p, P.lg[j]);
    for (int64_t s = 0; s < S; ++s) {
      const std::complex<double> w = toeplitz_root((k1 * s) % N, N);
      out[2 * (p * S + s)] = (F)w.real(), out[2 * (p * S + s) + 1] = (F)w.imag();
    }
  }
}

// ---- the device side (slq_toeplitz.hip) ----
// One product of one panel: T[rows < n] = A W[rows < n]. W, T: the panel's n rows of pw reals; ws: L pw reals (levels > 1). col0: the
// panel's first column among the plan's; columns >= nprobes enter as zeros (a padding column would otherwise reach its pair).
struct ToeplitzLaunch {
  const void *W = nullptr;
  void *T = nullptr, *ws = nullptr;
  const void *sym = nullptr, *tab = nullptr, *tw[2] = {nullptr, nullptr};
  int pw = 0, col0 = 0, nprobes = 0;
};
// raises the dynamic-LDS limit of every kernel (once per process and device; outside any capture). false: hipFuncSetAttribute failed.
bool toeplitz_prepare();
// 0: every launch was issued. kToeplitzBadGeometry: the panel width is no multiple of a workgroup's columns (nothing was launched). Otherwise the
// hipError_t of the failed launch, as an int (hipGetLastError has been consumed: the caller reports this value).
constexpr int kToeplitzBadGeometry = -1;
int toeplitz_launch(int dtype_is_f64, const ToeplitzPlan &P, const ToeplitzLaunch &a, void *stream);

}  // namespace slq
