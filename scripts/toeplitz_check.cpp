// toeplitz_check.cpp — the host side of the Toeplitz operator (primate_amd/csrc/slq_toeplitz.hpp) without a device.
//   toeplitz_check symbol N RHO_C RHO_R   writes L, then FFT_L(e) of c = RHO_C^k, r = RHO_R^k as 2 L doubles (binary) to stdout:
//                                         tests/test_toeplitz_cpu.py compares it with numpy.fft.fft
//   toeplitz_check passes N [f32]         runs the pass structure of a product on the host - the same tiles, the same index arithmetic,
//                                         the same tables as the kernels of slq_toeplitz.hip, in the operator's precision - on one
//                                         group of complex columns and compares with the O(n^2) product in long double; exit 1 when a
//                                         column misses eps log2(L) |t|_1 |pair|_2
// Build: c++ -O2 -std=c++17 scripts/toeplitz_check.cpp -o toeplitz_check (add -fsanitize=address,undefined for the sanitizer run).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "../primate_amd/csrc/slq_toeplitz.hpp"

using namespace slq;

template <typename F> struct Cx {
  F x, y;
};
template <typename F> static Cx<F> mul(Cx<F> a, Cx<F> b) { return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
template <typename F> static Cx<F> mulc(Cx<F> a, Cx<F> b) { return {a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y}; }

// tz_fft_lds, one column
template <typename F> static void fft_tile(std::vector<Cx<F>> &x, const Cx<F> *wt, bool inv, bool tfast, int lg_m, int lg_t, int si, int st) {
  const int lg_half = lg_m - 1, total = 1 << (lg_half + lg_t);
  for (int s = 0; s < lg_m; ++s) {
    const int lh = inv ? s : lg_m - 1 - s, h = 1 << lh;
    for (int id = 0; id < total; ++id) {
      const int j = tfast ? id >> lg_t : id & ((1 << lg_half) - 1);
      const int t = tfast ? id & ((1 << lg_t) - 1) : id >> lg_half;
      const int off = j & (h - 1), i0 = ((j >> lh) << (lh + 1)) + off;
      const size_t r0 = (size_t)(i0 * si + t * st), r1 = r0 + (size_t)h * si;
      if (r1 >= x.size() || (off << (9 - lh)) >= kToeplitzTab / 2) { fprintf(stderr, "tile index out of range\n"); exit(2); }
      const Cx<F> w = wt[off << (9 - lh)], a = x[r0], b = x[r1];
      if (inv) {
        const Cx<F> bw = mulc(b, w);
        x[r0] = {a.x + bw.x, a.y + bw.y}, x[r1] = {a.x - bw.x, a.y - bw.y};
      } else {
        x[r0] = {a.x + b.x, a.y + b.y}, x[r1] = mul(Cx<F>{a.x - b.x, a.y - b.y}, w);
      }
    }
  }
}

template <typename F> static int run_passes(int64_t n) {
  const ToeplitzPlan P = toeplitz_plan(n, (int)sizeof(F), 32);
  std::vector<double> c((size_t)n), r((size_t)n), cr, rr;
  for (int64_t k = 0; k < n; ++k) c[(size_t)k] = std::pow(0.5, (double)k), r[(size_t)k] = std::pow(0.3, (double)k);
  bool sym;
  char msg[160];
  if (!toeplitz_round_values(n, (int)sizeof(F), c.data(), r.data(), cr, rr, &sym, msg, sizeof msg)) return 2;
  const auto s = toeplitz_symbol(P, cr, rr);
  std::vector<Cx<F>> symd((size_t)P.L), tab(kToeplitzTab / 2), tw[2];
  toeplitz_device_symbol<F>(P, s, (F *)symd.data());
  toeplitz_device_tab<F>((F *)tab.data());
  int lg_s[3];
  for (int j = 0; j < P.levels; ++j) lg_s[j] = (int)toeplitz_level_stride_log2(P, j);
  for (int j = 0; j + 1 < P.levels; ++j) {
    tw[j].resize((size_t)1 << (P.lg[j] + lg_s[j]));
    toeplitz_device_twiddles<F>(P, j, (F *)tw[j].data());
  }
  std::mt19937_64 g(7);
  std::normal_distribution<double> nd;
  std::vector<Cx<F>> W((size_t)n), T((size_t)n, Cx<F>{0, 0}), ws((size_t)(P.levels > 1 ? P.L : 0));
  for (auto &v : W) v = {(F)nd(g), (F)nd(g)};
  auto panel = [&](int64_t pos) { return pos < n ? W[(size_t)pos] : Cx<F>{0, 0}; };
  auto outer = [&](int j, bool inv, bool is_panel) {
    const int lg_m = P.lg[j], lg_t = toeplitz_log2_ceil(P.tile_rows[j]) - lg_m, rows = 1 << (lg_m + lg_t);
    if (lg_t > lg_s[j]) { fprintf(stderr, "tile wider than a block\n"); exit(2); }
    std::vector<Cx<F>> x((size_t)rows);
    for (int64_t bx = 0; bx < P.L / rows; ++bx) {
      const int64_t block = bx >> (lg_s[j] - lg_t), s0 = (bx & ((1 << (lg_s[j] - lg_t)) - 1)) << lg_t, base = (block << (lg_m + lg_s[j])) + s0;
      for (int row = 0; row < rows; ++row) {
        const int p = row >> lg_t, t = row & ((1 << lg_t) - 1);
        const int64_t pos = base + ((int64_t)p << lg_s[j]) + t, ti = ((int64_t)p << lg_s[j]) + s0 + t;
        if (pos >= P.L || ti >= (int64_t)tw[j].size()) { fprintf(stderr, "outer index out of range\n"); exit(2); }
        x[(size_t)row] = !inv ? (is_panel ? panel(pos) : ws[(size_t)pos]) : mulc(ws[(size_t)pos], tw[j][(size_t)ti]);
      }
      fft_tile<F>(x, tab.data(), inv, true, lg_m, lg_t, 1 << lg_t, 1);
      for (int row = 0; row < rows; ++row) {
        const int p = row >> lg_t, t = row & ((1 << lg_t) - 1);
        const int64_t pos = base + ((int64_t)p << lg_s[j]) + t, ti = ((int64_t)p << lg_s[j]) + s0 + t;
        if (!inv) ws[(size_t)pos] = mul(x[(size_t)row], tw[j][(size_t)ti]);
        else if (!is_panel) ws[(size_t)pos] = x[(size_t)row];
        else if (pos < n) T[(size_t)pos] = x[(size_t)row];
      }
    }
  };
  auto mid = [&](bool is_panel) {
    const int j = P.levels - 1, lg_m = P.lg[j], lg_t = toeplitz_log2_ceil(P.tile_rows[j]) - lg_m, rows = 1 << (lg_m + lg_t);
    std::vector<Cx<F>> x((size_t)rows);
    for (int64_t bx = 0; bx < P.L / rows; ++bx) {
      const int64_t base = bx * rows;
      for (int row = 0; row < rows; ++row) x[(size_t)row] = is_panel ? panel(base + row) : ws[(size_t)(base + row)];
      fft_tile<F>(x, tab.data(), false, false, lg_m, lg_t, 1, 1 << lg_m);
      for (int row = 0; row < rows; ++row) x[(size_t)row] = mul(x[(size_t)row], symd[(size_t)(base + row)]);
      fft_tile<F>(x, tab.data(), true, false, lg_m, lg_t, 1, 1 << lg_m);
      for (int row = 0; row < rows; ++row) {
        if (!is_panel) ws[(size_t)(base + row)] = x[(size_t)row];
        else if (base + row < n) T[(size_t)(base + row)] = x[(size_t)row];
      }
    }
  };
  if (P.levels == 1) mid(true);
  else {
    outer(0, false, true);
    if (P.levels == 3) outer(1, false, false);
    mid(false);
    if (P.levels == 3) outer(1, true, false);
    outer(0, true, true);
  }
  // the model in long double, over the band where the values are not exact zeros
  long double t1 = 0, e2[2] = {0, 0}, pn = 0;
  for (int64_t k = 0; k < n; ++k) t1 += fabsl((long double)cr[(size_t)k]) + (k ? fabsl((long double)rr[(size_t)k]) : 0);
  for (int64_t i = 0; i < n; ++i) {
    long double yr = 0, yi = 0;
    for (int64_t jj = (i > 1100 ? i - 1100 : 0); jj < n && jj <= i + 1100; ++jj) {  // (0.5^k and 0.3^k are exact zeros in double beyond k = 1075)
      const long double a = i >= jj ? cr[(size_t)(i - jj)] : rr[(size_t)(jj - i)];
      if (a == 0) continue;
      yr += a * W[(size_t)jj].x, yi += a * W[(size_t)jj].y;
    }
    e2[0] += (T[(size_t)i].x - yr) * (T[(size_t)i].x - yr), e2[1] += (T[(size_t)i].y - yi) * (T[(size_t)i].y - yi);
    pn += (long double)W[(size_t)i].x * W[(size_t)i].x + (long double)W[(size_t)i].y * W[(size_t)i].y;
  }
  const long double eps = sizeof(F) == 8 ? ldexpl(1, -53) : ldexpl(1, -24), bar = eps * P.log2L * t1 * sqrtl(pn);
  const double worst = (double)(sqrtl(e2[0] > e2[1] ? e2[0] : e2[1]) / bar);
  printf("n %lld L %lld levels %d lengths %d %d %d worst/bar %.3f\n", (long long)n, (long long)P.L, P.levels, 1 << P.lg[0], P.levels > 1 ? 1 << P.lg[1] : 1,
         P.levels > 2 ? 1 << P.lg[2] : 1, worst);
  return worst <= 1.0 ? 0 : 1;
}

int main(int argc, char **argv) {
  if (argc >= 5 && !strcmp(argv[1], "symbol")) {
    const int64_t n = atoll(argv[2]);
    const double pc = atof(argv[3]), pr = atof(argv[4]);
    if (n < 1 || n > kToeplitzMaxN) return 2;
    const ToeplitzPlan P = toeplitz_plan(n, 8, 16);
    std::vector<double> c((size_t)n), r((size_t)n);
    for (int64_t k = 0; k < n; ++k) c[(size_t)k] = std::pow(pc, (double)k), r[(size_t)k] = std::pow(pr, (double)k);
    const auto s = toeplitz_symbol(P, c, r);
    const double L = (double)P.L;
    fwrite(&L, 8, 1, stdout);
    fwrite(s.data(), 16, s.size(), stdout);
    return 0;
  }
  if (argc >= 3 && !strcmp(argv[1], "passes")) {
    const int64_t n = atoll(argv[2]);
    if (n < 1 || n > kToeplitzMaxN) return 2;
    return argc >= 4 && !strcmp(argv[3], "f32") ? run_passes<float>(n) : run_passes<double>(n);
  }
  fprintf(stderr, "usage: toeplitz_check symbol N RHO_C RHO_R | passes N [f32]\n");
  return 2;
}
