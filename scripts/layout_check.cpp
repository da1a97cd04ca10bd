// layout_check.cpp — the host analysis of an operator's creation (csrc/slq_layout.hpp: no HIP dependency) as a stand-alone host
// program, for the sanitizers: prefilter, layout, permuted CSR, upper triangle, tile lists, tile streams (R = 1, and R = 2, 4 on
// merged boundaries, padded and unpadded), regrouped upper tiles - on a 5-point grid 96^2, a 7-point grid 24^3 (fp64 and fp32), a
// 22^3 grid with non-symmetric weights and a random symmetric graph of 6000 rows; every output checked against its definition
// and compared byte for byte between 1 and 8 host threads.
//   c++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=all scripts/layout_check.cpp -o layout_check && ./layout_check
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <string>

#include "../primate_amd/csrc/slq_layout.hpp"

using namespace slq;

static const char *g_case = "";
#define CHECK(cond)                                                                     \
  do {                                                                                  \
    if (!(cond)) {                                                                      \
      fprintf(stderr, "%s: %s fails (line %d)\n", g_case, #cond, __LINE__);             \
      exit(1);                                                                          \
    }                                                                                   \
  } while (0)

struct Matrix {
  int64_t n = 0;
  std::vector<int32_t> rp, ci;
  std::vector<double> va;
  bool symmetric = true;
};
static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // (xorshift64*)
  g_rng ^= g_rng >> 12, g_rng ^= g_rng << 25, g_rng ^= g_rng >> 27;
  return g_rng * 0x2545F4914F6CDD1Dull;
}
static Matrix from_rows(const std::vector<std::map<int32_t, double>> &rows, bool symmetric) {
  Matrix M;
  M.n = (int64_t)rows.size(), M.symmetric = symmetric;
  M.rp.push_back(0);
  for (auto &r : rows) {
    for (auto &e : r) M.ci.push_back(e.first), M.va.push_back(e.second);
    M.rp.push_back((int32_t)M.ci.size());
  }
  return M;
}
// the (2 d + 1)-point grid of m^d nodes; weights: 0 the Laplacian, 1 random and not symmetric
static Matrix grid(int m, int d, int weights) {
  int64_t n = 1;
  for (int k = 0; k < d; ++k) n *= m;
  std::vector<std::map<int32_t, double>> rows((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    double sum = 0.0;
    for (int64_t k = 0, stride = 1; k < d; ++k, stride *= m) {
      const int64_t c = (i / stride) % m;
      for (int s = -1; s <= 1; s += 2)
        if (c + s >= 0 && c + s < m) {
          const double w = weights ? 0.5 + (double)(rnd() >> 11) / 9007199254740992.0 : 1.0;
          rows[(size_t)i][(int32_t)(i + s * stride)] = -w, sum += w;
        }
    }
    rows[(size_t)i][(int32_t)i] = weights ? sum + 1.0 : 2.0 * d;
  }
  return from_rows(rows, weights == 0);
}
static Matrix random_graph(int64_t n, int per_row) {
  std::vector<std::map<int32_t, double>> rows((size_t)n);
  for (int64_t e = 0; e < n * per_row / 2; ++e) {
    const int32_t i = (int32_t)(rnd() % (uint64_t)n), j = (int32_t)(rnd() % (uint64_t)n);
    if (i == j) continue;
    const double w = 0.5 + (double)(rnd() >> 11) / 9007199254740992.0;
    rows[(size_t)i][j] = w, rows[(size_t)j][i] = w;
  }
  for (int64_t i = 0; i < n; ++i) rows[(size_t)i][(int32_t)i] = 10.0;
  return from_rows(rows, true);
}

// every buffer a run produced, by name: compared between thread counts
typedef std::map<std::string, std::vector<char>> Outputs;
template <typename T> static void keep(Outputs &out, const std::string &name, const T *p, size_t count) {
  const char *b = (const char *)p;
  CHECK(!out.count(name));
  out[name].assign(b, b + count * sizeof(T));
}
template <typename T> static void keep(Outputs &out, const std::string &name, const std::vector<T> &v) { keep(out, name, v.data(), v.size()); }

static int32_t padded(int32_t cnt) { return std::max<int32_t>(4, (cnt + 3) / 4 * 4); }

static void check_layout(const Matrix &M, const OperatorSwitches &osw, bool plain, const LayoutPrefilter &pre, const OperatorLayout &L) {
  const int64_t n = M.n, chunk = (n + 7) / 8;
  CHECK(L.perm.empty() == L.inv.empty() && L.perm.empty() == L.rowptr_stored.empty());
  if (!L.perm.empty()) {
    CHECK((int64_t)L.perm.size() == n && (int64_t)L.inv.size() == n && (int64_t)L.rowptr_stored.size() == n + 1);
    std::vector<char> hit((size_t)n, 0);
    for (int64_t i = 0; i < n; ++i) {
      CHECK(L.perm[(size_t)i] >= 0 && L.perm[(size_t)i] < n && !hit[(size_t)L.perm[(size_t)i]]);
      hit[(size_t)L.perm[(size_t)i]] = 1;
      CHECK(L.inv[(size_t)L.perm[(size_t)i]] == i);
      CHECK(L.perm[(size_t)i] / chunk == i / chunk);  // (rows never leave their XCD chunk)
      CHECK(L.rowptr_stored[(size_t)i + 1] - L.rowptr_stored[(size_t)i] == M.rp[(size_t)L.perm[(size_t)i] + 1] - M.rp[(size_t)L.perm[(size_t)i]]);
    }
    CHECK(L.rowptr_stored[0] == 0);
  }
  if (plain) CHECK(L.perm.empty() && !L.have_tiles && pre.reorder_mode == 0 && pre.tmode == 0);
  if (n < 4096) CHECK(!pre.try_tiles);
  if (!pre.try_tiles) CHECK(!L.have_tiles);
  for (int x = 0; x < 8; ++x) CHECK(L.xcd_tile[x] <= L.xcd_tile[x + 1]);
  if (!L.have_tiles) {
    CHECK(L.tile_row.empty() && L.xcd_tile[8] == 0);
    return;
  }
  CHECK(!L.perm.empty());
  const size_t ntiles = L.tile_row.size() - 1;
  CHECK(L.xcd_tile[8] == (int32_t)ntiles && L.tile_row[0] == 0 && L.tile_row[ntiles] == n);
  for (int x = 0; x <= 8; ++x) CHECK(L.tile_row[(size_t)L.xcd_tile[x]] == std::min<int64_t>(n, x * chunk));
  const bool ringed = osw.tiles == 2;
  for (size_t t = 0; t < ntiles; ++t) {
    const int32_t r0 = L.tile_row[t], r1 = L.tile_row[t + 1];
    CHECK(r0 < r1 && r0 / chunk == (r1 - 1) / chunk);
    std::set<int32_t> lines;
    int32_t nz = 0;
    for (int32_t r = r0; r < r1; ++r) {
      lines.insert(r);
      const int32_t o = L.perm[(size_t)r];
      for (int32_t q = M.rp[(size_t)o]; q < M.rp[(size_t)o + 1]; ++q) lines.insert(L.inv[(size_t)M.ci[(size_t)q]]), ++nz;
    }
    if (ringed) CHECK(r1 - r0 <= kRingTileRows && (int)lines.size() <= kRingTileCols && nz <= kRingTileNnz);
    else CHECK(r1 - r0 <= osw.tile_rows && (int)lines.size() <= osw.tile_cols);
  }
}

// a tile stream against what it is made from
template <typename F>
static void check_stream(int R, bool pad, int64_t n, const int32_t *rp, const int32_t *ci, const F *va, const std::vector<int32_t> &tile_row, const std::vector<int32_t> &tp,
                         const std::vector<int32_t> &tc, const RawBuf<int32_t> &desc, const RawBuf<char> &rec) {
  const size_t ntiles = tile_row.size() - 1, dw = (size_t)64 * R;
  CHECK(desc.size() == ntiles * dw && tile_row[ntiles] == n);
  for (size_t t = 0; t < ntiles; ++t) {
    const int32_t *d = desc.data() + t * dw;
    const int32_t r0 = tile_row[t], rows = tile_row[t + 1] - r0, D = tp[t + 1] - tp[t];
    CHECK(d[kDescRow0] == r0 && d[kDescRows] == rows && d[kDescCols] == D);
    for (int32_t c = 0; c < D; ++c) {
      const int32_t line = R == 1 ? d[kDescList + ring1_list_pos(c)] : d[(size_t)(c % R) * 64 + kDescList + c / R];
      CHECK(line == tc[(size_t)tp[t] + c]);
    }
    const size_t off = (size_t)d[kDescRecOff] * 16, bytes = (size_t)d[kDescRecChunks] * 1024;
    CHECK(off + bytes <= rec.size());  // (a record is fetched in whole KiB: the spare record behind the last one covers it)
    const int32_t *head = (const int32_t *)(rec.data() + off);
    const int32_t *lc = (const int32_t *)(rec.data() + off + (size_t)kRecHeadBytes * R);
    const F *v = (const F *)(rec.data() + off + head[16 * R - 1]);
    CHECK(head[0] == 0);
    for (int32_t i = 0; i < rows; ++i) {
      const int32_t q0 = rp[r0 + i], cnt = rp[r0 + i + 1] - q0, self = head[16 * R + i];
      CHECK(self >= 0 && self < D && tc[(size_t)tp[t] + self] == r0 + i);
      CHECK(head[i + 1] - head[i] == (pad ? padded(cnt) : cnt));
      for (int32_t q = 0; q < head[i + 1] - head[i]; ++q) {
        const int32_t l = lc[head[i] + q];
        CHECK(l >= 0 && l < D);
        if (q < cnt) CHECK(tc[(size_t)tp[t] + l] == ci[q0 + q] && v[head[i] + q] == va[q0 + q]);
        else CHECK(l == self && v[head[i] + q] == (F)0);
      }
    }
  }
}

template <typename F>
static void lists_and_stream(Outputs &out, const std::string &tag, int R, int want_pad, int64_t n, const int32_t *rp, const int32_t *ci, const F *va,
                             const std::vector<int32_t> &tile_row, const OperatorSwitches &osw, int cap) {
  std::vector<int32_t> tp, tc, lc, si;
  int mx = 0;
  build_tile_meta(n, rp, ci, tile_row, tp, tc, lc, si, &mx, osw);
  const size_t ntiles = tile_row.size() - 1;
  CHECK(tp.size() == ntiles + 1 && tc.size() == (size_t)tp[ntiles] + kCsrPad && lc.size() == (size_t)rp[n] + kCsrPad && (int64_t)si.size() == n && mx <= cap);
  int longest = 0;
  for (size_t t = 0; t < ntiles; ++t) {
    const int32_t *list = tc.data() + tp[t];
    const int32_t D = tp[t + 1] - tp[t];
    longest = std::max(longest, (int)D);
    for (int32_t c = 1; c < D; ++c) CHECK(list[c - 1] < list[c]);  // sorted, duplicate-free
    for (int32_t r = tile_row[t]; r < tile_row[t + 1]; ++r) {       // ... and holding every row and every column of its rows
      CHECK(si[(size_t)r] >= 0 && si[(size_t)r] < D && list[si[(size_t)r]] == r);
      for (int32_t q = rp[r]; q < rp[r + 1]; ++q) CHECK(lc[(size_t)q] >= 0 && lc[(size_t)q] < D && list[lc[(size_t)q]] == ci[q]);
    }
  }
  CHECK(longest == mx);
  keep(out, tag + "/tile_ptr", tp), keep(out, tag + "/tile_cols", tc), keep(out, tag + "/lcol", lc), keep(out, tag + "/self_idx", si);
  if (osw.tiles != 2) return;
  for (int p = 0; p <= want_pad; ++p) {
    RawBuf<int32_t> desc;
    RawBuf<char> rec;
    bool pad = p != 0;
    build_ring_stream<F>(R, rp, va, tile_row, tp, tc, lc, si, desc, rec, p ? &pad : nullptr);
    check_stream<F>(R, pad, n, rp, ci, va, tile_row, tp, tc, desc, rec);
    const std::string name = tag + (p ? (pad ? "/padded" : "/pad declined") : "/unpadded");
    keep(out, name + "/desc", desc.data(), desc.size()), keep(out, name + "/rec", rec.data(), rec.size());
  }
}

template <typename F> static Outputs run(const Matrix &M, OperatorSwitches osw, bool plain) {
  Outputs out;
  const int64_t n = M.n, nnz = (int64_t)M.ci.size();
  std::vector<F> vals(M.va.begin(), M.va.end());
  const CsrView A{n, nnz, M.rp.data(), M.ci.data()};
  const LayoutPrefilter pre = layout_prefilter(A, osw, plain);
  const OperatorLayout L = decide_layout(A, osw, pre, nullptr);
  check_layout(M, osw, plain, pre, L);
  keep(out, "perm", L.perm), keep(out, "inv", L.inv), keep(out, "rowptr_stored", L.rowptr_stored), keep(out, "tile_row", L.tile_row);
  keep(out, "xcd_tile", L.xcd_tile, 9), keep(out, "rms_dist", &L.rms_dist, 1);
  // the stored CSR: A' = P A P^T, every row sorted by its new columns
  std::vector<int32_t> rp(M.rp), ci(M.ci);
  std::vector<F> va(vals);
  if (!L.perm.empty()) {
    rp = L.rowptr_stored;
    for (int64_t i = 0; i < n; ++i) {
      const int32_t o = L.perm[(size_t)i];
      std::vector<std::pair<int32_t, int32_t>> row;
      for (int32_t q = M.rp[(size_t)o]; q < M.rp[(size_t)o + 1]; ++q) row.emplace_back(L.inv[(size_t)M.ci[(size_t)q]], q);
      std::sort(row.begin(), row.end());
      for (size_t k = 0; k < row.size(); ++k) ci[(size_t)rp[(size_t)i] + k] = row[k].first, va[(size_t)rp[(size_t)i] + k] = vals[(size_t)row[k].second];
    }
  }
  // the upper triangle against a naive one; absent for the non-symmetric matrix
  std::vector<int32_t> urp, uci;
  std::vector<char> uva;
  const bool sym = !plain && build_symmetric_upper<F>(n, rp.data(), ci.data(), va.data(), urp, uci, uva);
  CHECK(plain || sym == M.symmetric);
  if (sym) {
    std::vector<int32_t> nrp(1, 0), nci;
    std::vector<F> nva;
    for (int64_t i = 0; i < n; ++i) {
      for (int32_t q = rp[(size_t)i]; q < rp[(size_t)i + 1]; ++q)
        if (ci[(size_t)q] >= i) nci.push_back(ci[(size_t)q]), nva.push_back(ci[(size_t)q] == i ? va[(size_t)q] : (F)2 * va[(size_t)q]);
      nrp.push_back((int32_t)nci.size());
    }
    CHECK(urp == nrp && uci == nci && uva.size() == nva.size() * sizeof(F) && memcmp(uva.data(), nva.data(), uva.size()) == 0);
    keep(out, "upper/rowptr", urp), keep(out, "upper/colind", uci), keep(out, "upper/vals", uva);
  }
  if (!L.have_tiles) return out;
  const bool ringed = osw.tiles == 2;
  lists_and_stream<F>(out, "full R=1", 1, 0, n, rp.data(), ci.data(), va.data(), L.tile_row, osw, ringed ? kRingTileCols : osw.tile_cols);
  if (!ringed) return out;
  // merged boundaries, chunk by chunk (ensure_ring_stream): R consecutive tiles of one XCD chunk
  std::vector<int32_t> mrow[2];
  for (int k = 0; k < 2; ++k) {
    const int R = 2 << k;
    for (int x = 0; x < 8; ++x)
      for (int32_t t = L.xcd_tile[x]; t < L.xcd_tile[x + 1]; t += R) mrow[k].push_back(L.tile_row[(size_t)t]);
    mrow[k].push_back((int32_t)n);
    lists_and_stream<F>(out, "full R=" + std::to_string(R), R, 0, n, rp.data(), ci.data(), va.data(), mrow[k], osw, kRingTileCols * R);
  }
  if (!sym) return out;
  // the upper-triangle stream's own tiles: runs of base tiles, within the caps, chunk by chunk - and the same from the caller's
  // CSR seen through the permutation (the device-side build's way)
  std::vector<int32_t> tile_row_u, tile_row_p;
  int32_t xcd_u[9], xcd_p[9];
  regroup_upper_tiles(urp.data(), uci.data(), L.tile_row, L.xcd_tile, tile_row_u, xcd_u);
  regroup_upper_tiles_permuted(M.rp.data(), M.ci.data(), L.perm, L.inv, L.tile_row, L.xcd_tile, tile_row_p, xcd_p);
  CHECK(tile_row_u == tile_row_p && memcmp(xcd_u, xcd_p, sizeof xcd_u) == 0);
  const size_t ntu = tile_row_u.size() - 1;
  CHECK(tile_row_u[0] == 0 && tile_row_u[ntu] == n && xcd_u[8] == (int32_t)ntu && ntu <= L.tile_row.size() - 1);
  for (int x = 0; x <= 8; ++x) CHECK(tile_row_u[(size_t)xcd_u[x]] == L.tile_row[(size_t)L.xcd_tile[x]]);
  for (size_t t = 0; t < ntu; ++t) {
    CHECK(tile_row_u[t] < tile_row_u[t + 1] && std::binary_search(L.tile_row.begin(), L.tile_row.end(), tile_row_u[t]));  // a run of base tiles
    std::set<int32_t> lines;
    int32_t pz = 0;
    for (int32_t r = tile_row_u[t]; r < tile_row_u[t + 1]; ++r) {
      lines.insert(r);
      for (int32_t q = urp[(size_t)r]; q < urp[(size_t)r + 1]; ++q) lines.insert(uci[(size_t)q]);
      pz += padded(urp[(size_t)r + 1] - urp[(size_t)r]);
    }
    const bool one_base_tile = *std::upper_bound(L.tile_row.begin(), L.tile_row.end(), tile_row_u[t]) == tile_row_u[t + 1];
    if (!one_base_tile) CHECK(tile_row_u[t + 1] - tile_row_u[t] <= kRingTileRows && (int)lines.size() <= kRingTileCols && pz <= kRingTileNnz);
  }
  keep(out, "upper/tile_row", tile_row_u), keep(out, "upper/xcd_tile", xcd_u, 9);
  CHECK(regroup_upper_wanted(osw, n, L.tile_row.size() - 1) == (osw.ring_upper_regroup != 0 && (double)n / (double)(L.tile_row.size() - 1) <= 0.8 * kRingTileRows));
  lists_and_stream<F>(out, "upper R=1", 1, 1, n, urp.data(), uci.data(), (const F *)uva.data(), tile_row_u, osw, kRingTileCols);
  for (int k = 0; k < 2; ++k)
    lists_and_stream<F>(out, "upper R=" + std::to_string(2 << k), 2 << k, 1, n, urp.data(), uci.data(), (const F *)uva.data(), mrow[k], osw, kRingTileCols * (2 << k));
  return out;
}

template <typename F> static void both_thread_counts(const char *name, const Matrix &M, const OperatorSwitches &osw, bool plain = false) {
  g_case = name;
  setenv("SLQ_HOST_THREADS", "1", 1);
  const Outputs a = run<F>(M, osw, plain);
  setenv("SLQ_HOST_THREADS", "8", 1);
  const Outputs b = run<F>(M, osw, plain);
  CHECK(a.size() == b.size());
  size_t bytes = 0;
  for (auto &e : a) {
    auto it = b.find(e.first);
    if (it == b.end() || it->second != e.second) {
      fprintf(stderr, "%s: %s differs between 1 and 8 host threads\n", name, e.first.c_str());
      exit(1);
    }
    bytes += e.second.size();
  }
  printf("%-44s ok: %zu buffers, %zu bytes, the same at 1 and 8 host threads\n", name, a.size(), bytes);
}

int main() {
  const Matrix g2 = grid(96, 2, 0), g3 = grid(24, 3, 0), g3w = grid(22, 3, 1), rg = random_graph(6000, 12), small = grid(40, 2, 0);
  OperatorSwitches t2;  // SLQ_TILES=2, set (operators below 65536 rows are tried only then)
  t2.tiles = 2, t2.tiles_forced = true;
  OperatorSwitches t1 = t2, t2r0 = t2, r2 = t2;
  t1.tiles = 1;
  t2r0.reorder = 0;
  r2.tiles = 0, r2.reorder = 2;
  both_thread_counts<double>("grid 96^2, fp64, tiles 2", g2, t2);
  both_thread_counts<double>("grid 24^3, fp64, tiles 2", g3, t2);
  both_thread_counts<float>("grid 24^3, fp32, tiles 2", g3, t2);
  both_thread_counts<double>("grid 22^3, non-symmetric weights, tiles 2", g3w, t2);
  both_thread_counts<double>("random graph n = 6000, tiles 2", rg, t2);
  both_thread_counts<double>("grid 96^2, tiles 1", g2, t1);
  both_thread_counts<double>("grid 24^3, tiles 2, reorder 0", g3, t2r0);
  both_thread_counts<double>("random graph n = 6000, reorder 2, tiles 0", rg, r2);
  both_thread_counts<double>("grid 24^3, reorder 2, tiles 0", g3, r2);
  both_thread_counts<double>("grid 96^2, plain", g2, t2, true);
  both_thread_counts<double>("grid 40^2 (n < 4096), tiles 2", small, t2);
  printf("layout_check: clean\n");
  return 0;
}
