// slq_toeplitz.hip — the product kernels of the Toeplitz operator (slq_toeplitz.hpp) in a translation unit of their
// own: 2 dtypes x {the last level from the panel / from the workspace, a forward and an inverse outer level from the panel / from
// the workspace} = 12 instantiations. The C-ABI over them (slq_toeplitz_*) is in slq.hip and calls toeplitz_prepare / toeplitz_launch.
//
// A workgroup of 256 threads owns CG complex columns (128 bytes of every row: 8 in fp64, 16 in fp32) and a tile of rows in LDS, row
// after row (row x CG complex: a lane group of CG lanes reads or writes one whole 128-byte row, in HBM and in LDS alike). The
// transforms inside LDS are radix 2 with one barrier per stage: decimation in frequency forward (natural in, bit-reversed out),
// decimation in time backward (bit-reversed in, natural out), roots from the W_1024 table in LDS. No atomics, nothing crosses a
// workgroup: a product is a pure function of its inputs, bit for bit.
#include <hip/hip_runtime.h>

#include <mutex>
#include <type_traits>

#include "slq_toeplitz.hpp"

namespace slq {

template <typename F> using tz_cx = typename std::conditional<sizeof(F) == 8, double2, float2>::type;

template <typename C> __device__ inline C tz_mul(C a, C b) { return C{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
template <typename C> __device__ inline C tz_mulc(C a, C b) { return C{a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y}; }  // a conj(b)

struct TzArgs {
  const void *W;   // panel in (PANEL kernels): n rows of hpw complex
  void *T;         // panel out
  void *ws;        // workspace: L rows of hpw complex
  const void *sym, *tab, *tw;
  int n, hpw, col0, nprobes;
  int lg_m;        // log2 of the transform length of this kernel
  int lg_t;        // log2 of the transforms side by side in a tile
  int lg_s;        // outer levels: log2 of the stride S between the points of a transform
};

// row of (point i, transform t) in the tile: i * si + t * st. TFAST: consecutive lane groups take consecutive t (si > 1), else consecutive points.
template <typename F, bool INV, bool TFAST> __device__ inline void tz_fft_lds(tz_cx<F> *x, const tz_cx<F> *wt, int lg_m, int lg_t, int si, int st) {
  using C = tz_cx<F>;
  constexpr int CG = kToeplitzRowBytes / (int)sizeof(C), NL = kToeplitzBlock / CG;
  const int c = threadIdx.x % CG, lane = threadIdx.x / CG;
  const int lg_half = lg_m - 1;
  const int total = 1 << (lg_half + lg_t);
  for (int s = 0; s < lg_m; ++s) {
    const int lh = INV ? s : lg_m - 1 - s;
    const int h = 1 << lh;
    for (int id = lane; id < total; id += NL) {
      const int j = TFAST ? id >> lg_t : id & ((1 << lg_half) - 1);
      const int t = TFAST ? id & ((1 << lg_t) - 1) : id >> lg_half;
      const int off = j & (h - 1);
      const int i0 = ((j >> lh) << (lh + 1)) + off;
      const int r0 = (i0 * si + t * st) * CG + c, r1 = r0 + h * si * CG;
      const C w = wt[off << (9 - lh)];  // W_{2h}^{off}
      const C a = x[r0], b = x[r1];
      if (INV) {
        const C bw = tz_mulc(b, w);
        x[r0] = C{a.x + bw.x, a.y + bw.y};
        x[r1] = C{a.x - bw.x, a.y - bw.y};
      } else {
        x[r0] = C{a.x + b.x, a.y + b.y};
        x[r1] = tz_mul(C{a.x - b.x, a.y - b.y}, w);
      }
    }
    __syncthreads();
  }
}

template <typename F> __device__ inline void tz_load_tab(tz_cx<F> *wt, const void *tab) {
  for (int t = threadIdx.x; t < kToeplitzTab / 2; t += kToeplitzBlock) wt[t] = ((const tz_cx<F> *)tab)[t];
}
// row `pos` of the panel, complex column q, with the columns at and beyond nprobes as zeros; rows >= n are zeros
template <typename F> __device__ inline tz_cx<F> tz_panel_load(const TzArgs &a, int64_t pos, int q) {
  using C = tz_cx<F>;
  if (pos >= a.n) return C{0, 0};
  C v = ((const C *)a.W)[pos * a.hpw + q];
  const int col = a.col0 + 2 * q;
  if (col >= a.nprobes) v.x = 0;
  if (col + 1 >= a.nprobes) v.y = 0;
  return v;
}

// The last level: tiles of 2^lg_t transforms of 2^lg_m consecutive positions. Forward, times the symbol, backward. PANEL: the only level
// (one tile, one transform): rows < n from W, rows < n to T.
template <typename F, bool PANEL> __global__ __launch_bounds__(kToeplitzBlock) void k_toeplitz_mid(TzArgs a) {
  using C = tz_cx<F>;
  constexpr int CG = kToeplitzRowBytes / (int)sizeof(C), NL = kToeplitzBlock / CG;
  extern __shared__ __align__(16) unsigned char tz_smem[];
  C *wt = (C *)tz_smem, *x = wt + kToeplitzTab / 2;
  const int c = threadIdx.x % CG, lane = threadIdx.x / CG;
  const int q = blockIdx.y * CG + c;
  const int rows = 1 << (a.lg_m + a.lg_t);
  const int64_t base = (int64_t)blockIdx.x * rows;
  tz_load_tab<F>(wt, a.tab);
  for (int row = lane; row < rows; row += NL) x[row * CG + c] = PANEL ? tz_panel_load<F>(a, base + row, q) : ((const C *)a.ws)[(base + row) * a.hpw + q];
  __syncthreads();
  tz_fft_lds<F, false, false>(x, wt, a.lg_m, a.lg_t, 1, 1 << a.lg_m);
  for (int row = lane; row < rows; row += NL) x[row * CG + c] = tz_mul(x[row * CG + c], ((const C *)a.sym)[base + row]);
  __syncthreads();
  tz_fft_lds<F, true, false>(x, wt, a.lg_m, a.lg_t, 1, 1 << a.lg_m);
  for (int row = lane; row < rows; row += NL) {
    const int64_t pos = base + row;
    if (PANEL) {
      if (pos < a.n) ((C *)a.T)[pos * a.hpw + q] = x[row * CG + c];
    } else {
      ((C *)a.ws)[pos * a.hpw + q] = x[row * CG + c];
    }
  }
}

// An outer level: blocks of 2^lg_m * S positions (S = 2^lg_s); a tile holds the transforms over p at 2^lg_t consecutive s of one block:
// row (p, t) <-> position block * 2^lg_m * S + p * S + s0 + t. Forward: load, transform, times tw[p * S + s], store to ws. Inverse: load
// from ws times the conjugate, transform, store. PANEL (the outermost level, one block): forward loads rows < n of W (zeros behind
// them), inverse stores rows < n to T.
template <typename F, bool INV, bool PANEL> __global__ __launch_bounds__(kToeplitzBlock) void k_toeplitz_outer(TzArgs a) {
  using C = tz_cx<F>;
  constexpr int CG = kToeplitzRowBytes / (int)sizeof(C), NL = kToeplitzBlock / CG;
  extern __shared__ __align__(16) unsigned char tz_smem[];
  C *wt = (C *)tz_smem, *x = wt + kToeplitzTab / 2;
  const int c = threadIdx.x % CG, lane = threadIdx.x / CG;
  const int q = blockIdx.y * CG + c;
  const int rows = 1 << (a.lg_m + a.lg_t);
  const int tiles_per_block = 1 << (a.lg_s - a.lg_t);
  const int64_t block = blockIdx.x >> (a.lg_s - a.lg_t);
  const int64_t s0 = (int64_t)(blockIdx.x & (tiles_per_block - 1)) << a.lg_t;
  const int64_t base = (block << (a.lg_m + a.lg_s)) + s0;
  const int tmask = (1 << a.lg_t) - 1;
  tz_load_tab<F>(wt, a.tab);
  for (int row = lane; row < rows; row += NL) {
    const int p = row >> a.lg_t, t = row & tmask;
    const int64_t pos = base + ((int64_t)p << a.lg_s) + t;
    C v;
    if (!INV) v = PANEL ? tz_panel_load<F>(a, pos, q) : ((const C *)a.ws)[pos * a.hpw + q];
    else v = tz_mulc(((const C *)a.ws)[pos * a.hpw + q], ((const C *)a.tw)[((int64_t)p << a.lg_s) + s0 + t]);
    x[row * CG + c] = v;
  }
  __syncthreads();
  tz_fft_lds<F, INV, true>(x, wt, a.lg_m, a.lg_t, 1 << a.lg_t, 1);
  for (int row = lane; row < rows; row += NL) {
    const int p = row >> a.lg_t, t = row & tmask;
    const int64_t pos = base + ((int64_t)p << a.lg_s) + t;
    const C v = x[row * CG + c];
    if (!INV) ((C *)a.ws)[pos * a.hpw + q] = tz_mul(v, ((const C *)a.tw)[((int64_t)p << a.lg_s) + s0 + t]);
    else if (!PANEL) ((C *)a.ws)[pos * a.hpw + q] = v;
    else if (pos < a.n) ((C *)a.T)[pos * a.hpw + q] = v;
  }
}

template <typename F> static bool toeplitz_prepare_dtype() {
  const int lim = 160 * 1024;
  hipError_t e = hipFuncSetAttribute((const void *)k_toeplitz_mid<F, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lim);
  if (e == hipSuccess) e = hipFuncSetAttribute((const void *)k_toeplitz_mid<F, false>, hipFuncAttributeMaxDynamicSharedMemorySize, lim);
  if (e == hipSuccess) e = hipFuncSetAttribute((const void *)k_toeplitz_outer<F, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lim);
  if (e == hipSuccess) e = hipFuncSetAttribute((const void *)k_toeplitz_outer<F, false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, lim);
  if (e == hipSuccess) e = hipFuncSetAttribute((const void *)k_toeplitz_outer<F, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lim);
  if (e == hipSuccess) e = hipFuncSetAttribute((const void *)k_toeplitz_outer<F, true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, lim);
  return e == hipSuccess;
}
bool toeplitz_prepare() {
  // per device: the attribute belongs to the function on the current device
  static std::mutex lock;
  static bool done[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
  std::lock_guard<std::mutex> g(lock);
  if (done[dev]) return true;
  if (!toeplitz_prepare_dtype<double>() || !toeplitz_prepare_dtype<float>()) return false;
  done[dev] = true;
  return true;
}

template <typename F> static int toeplitz_launch_dtype(const ToeplitzPlan &P, const ToeplitzLaunch &l, hipStream_t st) {
  using C = tz_cx<F>;
  const int hpw = l.pw / 2;
  if (hpw < P.cg || hpw % P.cg != 0) return kToeplitzBadGeometry;
  const unsigned gy = (unsigned)(hpw / P.cg);
  const size_t row = (size_t)P.cg * sizeof(C), tab = (size_t)(kToeplitzTab / 2) * sizeof(C);
  TzArgs a{l.W, l.T, l.ws, l.sym, l.tab, nullptr, (int)P.n, hpw, l.col0, l.nprobes, 0, 0, 0};
  auto lds = [&](int j) { return (size_t)P.tile_rows[j] * row + tab; };
  auto tiles = [&](int j) { return (unsigned)(P.L / P.tile_rows[j]); };
  auto lg_of = [](int v) { return toeplitz_log2_ceil(v); };
  const int last = P.levels - 1;
  // the strides of the outer levels
  int lg_s[3] = {0, 0, 0};
  for (int j = 0; j < P.levels; ++j) lg_s[j] = (int)toeplitz_level_stride_log2(P, j);
  auto outer_args = [&](int j) {
    TzArgs b = a;
    b.tw = l.tw[j], b.lg_m = P.lg[j], b.lg_t = lg_of(P.tile_rows[j]) - P.lg[j], b.lg_s = lg_s[j];
    return b;
  };
  if (P.levels == 1) {
    a.lg_m = P.lg[0], a.lg_t = 0;
    k_toeplitz_mid<F, true><<<dim3(1, gy), dim3(kToeplitzBlock), lds(0), st>>>(a);
    return (int)hipGetLastError();
  }
  k_toeplitz_outer<F, false, true><<<dim3(tiles(0), gy), dim3(kToeplitzBlock), lds(0), st>>>(outer_args(0));
  if (P.levels == 3) k_toeplitz_outer<F, false, false><<<dim3(tiles(1), gy), dim3(kToeplitzBlock), lds(1), st>>>(outer_args(1));
  a.lg_m = P.lg[last], a.lg_t = lg_of(P.tile_rows[last]) - P.lg[last];
  k_toeplitz_mid<F, false><<<dim3(tiles(last), gy), dim3(kToeplitzBlock), lds(last), st>>>(a);
  if (P.levels == 3) k_toeplitz_outer<F, true, false><<<dim3(tiles(1), gy), dim3(kToeplitzBlock), lds(1), st>>>(outer_args(1));
  k_toeplitz_outer<F, true, true><<<dim3(tiles(0), gy), dim3(kToeplitzBlock), lds(0), st>>>(outer_args(0));
  return (int)hipGetLastError();
}

int toeplitz_launch(int dtype_is_f64, const ToeplitzPlan &P, const ToeplitzLaunch &a, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  return dtype_is_f64 ? toeplitz_launch_dtype<double>(P, a, st) : toeplitz_launch_dtype<float>(P, a, st);
}

}  // namespace slq
