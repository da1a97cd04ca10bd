// slq_layout.hpp — the host analysis of a CSR operator's creation: row order, clusters, tile lists, tile streams, upper triangle,
// and on top of them the decision itself as a value (layout_prefilter, decide_layout -> OperatorLayout). Plain C++ (no HIP
// include, no HIP call): it runs without a device - slq_debug_csr_layout, tests/test_layout_cpu.py, scripts/layout_check.cpp (the
// program to run under a sanitizer). slq.hip's csr_create_body runs the phases in order and hands the layout to one of its two
// storage builders (build_storage_host, build_storage_device).
#pragma once

#include <stdint.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <new>
#include <thread>
#include <utility>
#include <vector>

#include "slq_format.hpp"
#include "slq_switches.hpp"

namespace slq {

constexpr double kTileMaxColsPerRow = 4.5;      // tiles are kept when a tile row needs at most this many distinct panel rows
constexpr double kTileAlphaColsPerRow = 2.6;    // upper-triangle tiles: the alpha-only pass takes the ring up to this many landed rows per row (r03: 7-point grids too)
constexpr double kTileAlphaMergedColsPerRow = 2.6;  // ... and on the merged tiles of narrow panels up to this many (of the unmerged tiles)
constexpr double kTileLevelRows = 320.0;        // level sets the tile sweep's base order should not exceed (decide_layout)

// Host-side work of an operator's creation (row orders, clusters, tile lists, streams) is cut into independent pieces -
// XCD chunks, tile ranges, row ranges - and run on a few threads: fn(piece, begin, end) over [0, count). Results never depend
// on the number of threads (every piece writes its own slots or its own buffer, joined in piece order). SLQ_HOST_THREADS
// overrides the default of min(16, hardware threads); it is the one switch read where it is used. Exceptions do not leave a worker: the first failure is reported.
inline int host_threads() {
  const int hw = (int)std::thread::hardware_concurrency();
  return std::max(1, std::min(64, or_auto(read_host_threads(), std::max(1, std::min(16, hw)))));
}
template <typename Fn> inline bool parallel_pieces(int pieces, int64_t count, Fn fn) {
  pieces = (int)std::max<int64_t>(1, std::min<int64_t>(pieces, count));
  const int64_t per = (count + pieces - 1) / pieces;
  if (pieces == 1) {
    try { fn(0, (int64_t)0, count); } catch (...) { return false; }
    return true;
  }
  std::vector<char> ok((size_t)pieces, 1);
  std::vector<std::thread> th;
  th.reserve((size_t)pieces);
  for (int t = 0; t < pieces; ++t) {
    const int64_t b = std::min(count, t * per), e = std::min(count, b + per);
    try {
      th.emplace_back([&, t, b, e]() {
        try { fn(t, b, e); } catch (...) { ok[(size_t)t] = 0; }
      });
    } catch (...) {  // no thread to be had: do the piece here
      try { fn(t, b, e); } catch (...) { ok[(size_t)t] = 0; }
    }
  }
  for (auto &x : th) x.join();
  return std::all_of(ok.begin(), ok.end(), [](char c) { return c != 0; });
}

// wall time of the phases of an operator's creation, printed under SLQ_DEBUG (scripts/time_create.py)
struct PhaseClock {
  bool on;
  explicit PhaseClock(const OperatorSwitches &sw) : on(sw.debug != 0) {}
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now(), t0 = t;
  void total(const char *what) {
    if (on) fprintf(stderr, "[slq] create: %-34s %7.1f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
  void lap(const char *what) {
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "[slq] create: %-34s %7.1f ms\n", what, std::chrono::duration<double, std::milli>(now - t).count());
    t = now;
  }
};

// Uninitialised host storage for the big arrays of an operator's creation (a std::vector zero-fills them on one thread,
// 20 ms per 100 MB, and every page is then touched a second time); whoever fills it writes every byte it will read.
template <typename T> struct RawBuf {
  std::unique_ptr<T[]> p;
  size_t n = 0;
  void alloc(size_t count) {
    p.reset(new T[count]);  // (default-initialised: no fill for arithmetic T)
    n = count;
  }
  T *data() { return p.get(); }
  const T *data() const { return p.get(); }
  size_t size() const { return n; }
};

// ---------------------------------------------------------------------------------------------------
// XCD-aware row reordering (speed only; results are permutation-invariant up to rounding)
// ---------------------------------------------------------------------------------------------------
// k_spmm_3term / k_csr_pass give XCD x the contiguous row range [x*n/8, (x+1)*n/8) and sweep it
// with all of the XCD's waves in lock-step, so a gathered panel row stays useful only while the
// sweep front is within the matrix bandwidth of it. With 1 KiB panel rows and a 4 MiB L2 the
// natural order of a 1000 x 1000 grid (bandwidth 1000 -> 2 MiB of halo) no longer fits beside the
// rows in flight: the alpha pass fetched 6.5 GB per launch against 4.2 GB algorithmic
// (profiles/r01b_pmc_per_kernel.csv). Reverse Cuthill-McKee INSIDE each XCD's chunk shrinks the
// bandwidth to the chunk's short dimension (125 for that grid; build/rcm_test in round 1). perm[new] = old.
// MEASURED RESULT: slower, see slq_csr_create. The L2 behaviour of this kernel is not explained by
// the reuse-distance model above (fewer resident workgroups also fetch MORE, not less).
// sub: second-level pieces per chunk (below). avg_level: if not null, receives the mean size of the breadth-first level sets of
// the final order - what a tile sweep has to keep in L2 between a row and its neighbours in the next level.
// first_level: the order a call with sub = 1 returned for this matrix (null: computed here) - the sweep over sub = 4, 16, 64 of
// decide_layout does the chunks' own Cuthill-McKee once (r04: it was redone per attempt, 12 ms of a 100^3 operator's creation).
inline void xcd_rcm_permutation(int64_t n, const int32_t *rowptr, const int32_t *colind, std::vector<int32_t> &perm, int sub,
                                double *avg_level, const std::vector<int32_t> *first_level = nullptr) {
  perm.resize((size_t)n);
  const int64_t chunk = (n + 7) / 8;
  // The eight chunks are independent: one worker each. deg / part / seen are indexed by node and a worker touches the
  // entries of its own chunk only (a neighbour's entry is read only after its index has been found inside the chunk).
  std::vector<int32_t> deg((size_t)n), part((size_t)n, -1);
  std::vector<char> seen((size_t)n, 0);
  sub = std::max(1, sub);
  int64_t levels_x[8] = {0, 0, 0, 0, 0, 0, 0, 0}, levelled_x[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  auto do_chunk = [&](int x) {
    const int64_t lo = x * chunk, hi = std::min<int64_t>(n, lo + chunk);
    if (lo >= hi) return;
    int64_t levels = 0, levelled = 0;  // of the committed searches since the last reset
    std::vector<int32_t> nbrs, order, members, first, piece, second;
    auto inside = [&](int32_t v, int32_t id) { return v >= lo && v < hi && part[(size_t)v] == id; };
    // Reverse Cuthill-McKee of the subgraph induced by `members` (all with part[v] == id), appended to `out`.
    auto rcm = [&](const std::vector<int32_t> &mem, int32_t id, std::vector<int32_t> &out) {
      for (int32_t v : mem) {
        int d = 0;
        for (int32_t p = rowptr[v]; p < rowptr[v + 1]; ++p) d += (colind[p] != v && inside(colind[p], id));
        deg[(size_t)v] = d;
      }
      order.clear();
      // candidates in increasing degree: starting points of the components
      std::vector<int32_t> cand(mem);
      std::stable_sort(cand.begin(), cand.end(), [&](int32_t a, int32_t b) { return deg[(size_t)a] < deg[(size_t)b]; });
      auto bfs = [&](int32_t start, bool commit, int32_t *last_min) {
        // breadth-first numbering with neighbours in increasing degree (Cuthill-McKee)
        const size_t base = order.size();
        order.push_back(start);
        seen[(size_t)start] = 1;
        size_t head = base, level_begin = base;
        while (head < order.size()) {
          const size_t level_end = order.size();
          level_begin = head;
          if (commit) {
            ++levels;
            levelled += (int64_t)(level_end - head);
          }
          for (; head < level_end; ++head) {
            const int32_t u = order[head];
            nbrs.clear();
            for (int32_t p = rowptr[u]; p < rowptr[u + 1]; ++p) {
              const int32_t v = colind[p];
              if (inside(v, id) && !seen[(size_t)v]) {
                seen[(size_t)v] = 1;
                nbrs.push_back(v);
              }
            }
            std::sort(nbrs.begin(), nbrs.end(), [&](int32_t a, int32_t b) { return deg[(size_t)a] < deg[(size_t)b] || (deg[(size_t)a] == deg[(size_t)b] && a < b); });
            order.insert(order.end(), nbrs.begin(), nbrs.end());
          }
        }
        // min-degree node of the last level: a pseudo-peripheral candidate
        int32_t far = order[level_begin];
        for (size_t q = level_begin; q < order.size(); ++q)
          if (deg[(size_t)order[q]] < deg[(size_t)far]) far = order[q];
        if (last_min) *last_min = far;
        if (!commit) {
          for (size_t q = base; q < order.size(); ++q) seen[(size_t)order[q]] = 0;
          order.resize(base);
        }
      };
      for (int32_t c : cand) {
        if (seen[(size_t)c]) continue;
        int32_t far = c;
        bfs(c, false, &far);      // one pseudo-peripheral refinement
        bfs(far, true, nullptr);
        // a pattern that is not symmetric: the search from `far` follows the stored entries only and need not lead back to c, which no
        // later pass of this loop would visit again - the order would come out short of the chunk (never taken for a symmetric pattern)
        if (!seen[(size_t)c]) bfs(c, true, nullptr);
      }
      for (int32_t v : mem) seen[(size_t)v] = 0;
      out.insert(out.end(), order.rbegin(), order.rend());  // reversed (RCM)
    };
    if (first_level && sub > 1) {
      first.assign(first_level->begin() + lo, first_level->begin() + hi);
    } else {
      members.resize((size_t)(hi - lo));
      for (int64_t i = lo; i < hi; ++i) {
        members[(size_t)(i - lo)] = (int32_t)i;
        part[(size_t)i] = x;
      }
      rcm(members, x, first);
    }
    // Second level (SLQ_RCM_SUB = K > 1): the chunk's RCM order is cut into K consecutive pieces of equal size - runs of
    // BFS levels, i.e. slices ACROSS the chunk's longest direction - and each piece is reordered on its own. A piece is
    // short along the old sweep direction, so its own Cuthill-McKee levels run along another one and are K times
    // smaller: the gather halo an XCD's L2 has to hold shrinks accordingly, at the price of the edges cut between pieces.
    if (sub > 1 && (int64_t)first.size() >= 64 * sub) {
      levels = levelled = 0;
      const size_t len = (first.size() + sub - 1) / sub;
      for (int k = 0; k < sub; ++k) {
        const size_t b0 = std::min(first.size(), k * len), b1 = std::min(first.size(), b0 + len);
        piece.assign(first.begin() + b0, first.begin() + b1);
        const int32_t id = 8 + x * sub + k;
        for (int32_t v : piece) part[(size_t)v] = id;
        rcm(piece, id, second);
      }
      first.swap(second);
    }
    levels_x[x] = levels;
    levelled_x[x] = levelled;
    for (int64_t q = 0; q < hi - lo; ++q) perm[(size_t)(lo + q)] = first[(size_t)q];
  };
  if (host_threads() > 1) {
    if (!parallel_pieces(8, 8, [&](int, int64_t x0, int64_t x1) { for (int64_t x = x0; x < x1; ++x) do_chunk((int)x); })) throw std::bad_alloc();
  } else {
    for (int x = 0; x < 8; ++x) do_chunk(x);
  }
  int64_t levels_all = 0, levelled_all = 0;
  for (int x = 0; x < 8; ++x) levels_all += levels_x[x], levelled_all += levelled_x[x];
  if (avg_level) *avg_level = levels_all > 0 ? (double)levelled_all / (double)levels_all : 0.0;
}


// Workgroup tiles for k_csr_tile_pass (SLQ_TILES). The rows of every XCD chunk are regrouped into compact clusters:
// seeds are taken in the chunk's current order (natural or Cuthill-McKee), a cluster grows breadth-first by the
// unassigned in-chunk neighbour with the most links into it (ties: first discovered), up to kTileRows rows and as long
// as its rows and columns together stay within kTileCols distinct indices. Clusters follow one another in seed order,
// so the sweep of the chunk keeps its locality. order_in: stored row -> caller row; inv_in: caller row -> stored row
// (null: identity). order_out: the new stored order; tile_row: first stored row of every tile; xcd_tile: tile range of
// every chunk. Returns false when a single row already needs more than kTileCols indices (no tiling for this operator).
// *lines_total (if not null): the sum over the clusters of their distinct indices (rows and columns) - the panel rows a sweep of the tiles lands.
inline bool build_clusters(int64_t n, const int32_t *rowptr, const int32_t *colind, const int32_t *order_in, const int32_t *inv_in,
                           std::vector<int32_t> &order_out, std::vector<int32_t> &tile_row, int32_t xcd_tile[9], const OperatorSwitches &osw, int64_t *lines_total = nullptr) {
  const int64_t chunk = (n + 7) / 8;
  const bool ringed = osw.tiles == 2;  // tiles of the ring-fed kernel (k_csr_ring_pass): smaller, fixed caps
  const int tmax = ringed ? kRingTileRows : std::max(1, std::min(osw.tile_rows, 64));
  const int dcap = ringed ? kRingTileCols : std::max(8, std::min(osw.tile_cols, kTileCols));
  const int nzcap = ringed ? kRingTileNnz : std::numeric_limits<int>::max();  // the ring kernel's tile record is bounded
  // The chunks are independent (a cluster never leaves its chunk): one worker each, with its own order, its own tile
  // boundaries (counted from the chunk's first row) and its own stamp array; `assigned` is shared, but a worker reads and
  // writes the entries of its own chunk's rows only.
  // (r03: every chunk is clustered as kClusterPieces independent halves of its order - a fixed split, so the tiles do not
  // depend on the number of host threads - because the greedy growth is sequential and was 25-50 ms of an operator's creation
  // with one worker per chunk; a cluster never crosses the middle of a chunk either: one short tile per 60,000 rows.)
  constexpr int kClusterPieces = 2, NX = 8 * kClusterPieces;
  std::vector<char> assigned((size_t)n, 0);
  std::vector<int32_t> order_x[NX], rows_x[NX];  // per piece: the new order, and the row count of every cluster
  int64_t lines_x[NX] = {};
  char failed[NX] = {};
  auto do_chunk = [&](int x) {
    const int64_t clo = (x / kClusterPieces) * chunk, chi = std::min<int64_t>(n, clo + chunk);
    if (clo >= chi) return;
    const int64_t plen = (chi - clo + kClusterPieces - 1) / kClusterPieces;
    const int64_t lo = clo + (x % kClusterPieces) * plen, hi = std::min<int64_t>(chi, lo + plen);
    if (lo >= hi) return;
    std::vector<int32_t> stamp((size_t)n, -1);
    struct Cand { int32_t node, cnt, disc; };
    std::vector<Cand> cand;
    // where a node of this piece sits in `cand` while it is a candidate of the current cluster (r04: the list was searched linearly for every
    // neighbour of every added row - 20 of the 35 ms this took on a 100^3 grid); indexed by position in the piece
    std::vector<int32_t> slot_of((size_t)(hi - lo), -1);
    std::vector<int32_t> &order = order_x[x];
    order.reserve((size_t)(hi - lo));
    int32_t cid = 0;
    auto in_chunk = [&](int32_t v) {
      const int64_t b = inv_in ? inv_in[v] : v;
      return b >= lo && b < hi;
    };
    for (int64_t b = lo; b < hi; ++b) {
      const int32_t seed = order_in ? order_in[b] : (int32_t)b;
      if (assigned[(size_t)seed]) continue;
      int D = 0, ndisc = 0, nz = 0;
      cand.clear();
      const size_t first_member = order.size();
      auto new_cols = [&](int32_t v) {
        int c = stamp[(size_t)v] != cid;
        for (int32_t p = rowptr[v]; p < rowptr[v + 1]; ++p) c += (stamp[(size_t)colind[p]] != cid && colind[p] != v);
        return c;
      };
      auto add = [&](int32_t v) {
        assigned[(size_t)v] = 1;
        order.push_back(v);
        nz += rowptr[v + 1] - rowptr[v];
        if (stamp[(size_t)v] != cid) { stamp[(size_t)v] = cid; ++D; }
        for (int32_t p = rowptr[v]; p < rowptr[v + 1]; ++p) {
          const int32_t c = colind[p];
          if (stamp[(size_t)c] != cid) { stamp[(size_t)c] = cid; ++D; }
          if (c != v && in_chunk(c) && !assigned[(size_t)c]) {
            int32_t &slot = slot_of[(size_t)((inv_in ? inv_in[c] : c) - lo)];
            if (slot >= 0) ++cand[(size_t)slot].cnt;
            else slot = (int32_t)cand.size(), cand.push_back(Cand{c, 1, ndisc++});
          }
        }
      };
      if (new_cols(seed) > dcap || rowptr[seed + 1] - rowptr[seed] > nzcap) { failed[x] = 1; return; }
      add(seed);
      while ((int)(order.size() - first_member) < tmax && !cand.empty()) {
        size_t best = 0;
        for (size_t q = 1; q < cand.size(); ++q)
          if (cand[q].cnt > cand[best].cnt || (cand[q].cnt == cand[best].cnt && cand[q].disc < cand[best].disc)) best = q;
        const int32_t v = cand[best].node;
        slot_of[(size_t)((inv_in ? inv_in[v] : v) - lo)] = -1;
        cand[best] = cand.back();
        cand.pop_back();
        if (best < cand.size()) slot_of[(size_t)((inv_in ? inv_in[cand[best].node] : cand[best].node) - lo)] = (int32_t)best;
        if (assigned[(size_t)v]) continue;
        if (D + new_cols(v) > dcap || nz + rowptr[v + 1] - rowptr[v] > nzcap) continue;  // would not fit: leave it for a later cluster
        add(v);
      }
      for (const Cand &k : cand) slot_of[(size_t)((inv_in ? inv_in[k.node] : k.node) - lo)] = -1;  // (what the cluster leaves behind)
      lines_x[x] += D;
      rows_x[x].push_back((int32_t)(order.size() - first_member));
      ++cid;
    }
  };
  if (host_threads() > 1) {
    if (!parallel_pieces(NX, NX, [&](int, int64_t x0, int64_t x1) { for (int64_t x = x0; x < x1; ++x) do_chunk((int)x); })) return false;
  } else {
    for (int x = 0; x < NX; ++x) do_chunk(x);
  }
  order_out.clear();
  order_out.reserve((size_t)n);
  tile_row.assign(1, 0);
  for (int x = 0; x < NX; ++x) {
    if (failed[x]) return false;
    if (x % kClusterPieces == 0) xcd_tile[x / kClusterPieces] = (int32_t)tile_row.size() - 1;
    order_out.insert(order_out.end(), order_x[x].begin(), order_x[x].end());
    for (int32_t r : rows_x[x]) tile_row.push_back(tile_row.back() + r);
  }
  xcd_tile[8] = (int32_t)tile_row.size() - 1;
  for (int x = 7; x >= 0; --x) xcd_tile[x] = std::min(xcd_tile[x], xcd_tile[x + 1]);
  if (lines_total) {
    *lines_total = 0;
    for (int x = 0; x < NX; ++x) *lines_total += lines_x[x];
  }
  return (int64_t)order_out.size() == n;
}

// A cheap look before the expensive one: grow one cluster from each of 256 evenly spaced seeds with build_clusters' rule (most
// links first, same caps) on the caller's numbering, and return the distinct panel rows per tile row of that sample. Operators
// whose rows share nothing (random graphs, bands with scattered far entries) show it here, in microseconds, and are spared the
// reorderings and the full clustering (tens of seconds at n = 10^7).
inline double sample_tile_quality(int64_t n, const int32_t *rowptr, const int32_t *colind, int tmax, int dcap, int nzcap) {
  const int64_t chunk = (n + 7) / 8;
  int64_t rows = 0, cols = 0;
  std::vector<int32_t> members, seen;
  struct Cand { int32_t node, cnt; };
  std::vector<Cand> cand;
  for (int sidx = 0; sidx < 256; ++sidx) {
    const int32_t seed = (int32_t)(((int64_t)sidx * n) / 256);
    const int64_t lo = (seed / chunk) * chunk, hi = std::min<int64_t>(n, lo + chunk);
    members.clear();
    seen.clear();
    cand.clear();
    int nz = 0;
    auto is_in = [](const std::vector<int32_t> &v, int32_t x) { return std::find(v.begin(), v.end(), x) != v.end(); };
    auto new_cols = [&](int32_t v) {
      int c = !is_in(seen, v);
      for (int32_t p = rowptr[v]; p < rowptr[v + 1]; ++p) c += (colind[p] != v && !is_in(seen, colind[p]));
      return c;
    };
    auto add = [&](int32_t v) {
      members.push_back(v);
      nz += rowptr[v + 1] - rowptr[v];
      if (!is_in(seen, v)) seen.push_back(v);
      for (int32_t p = rowptr[v]; p < rowptr[v + 1]; ++p) {
        const int32_t c = colind[p];
        if (!is_in(seen, c)) seen.push_back(c);
        if (c != v && c >= lo && c < hi && !is_in(members, c)) {
          bool found = false;
          for (auto &k : cand) if (k.node == c) { ++k.cnt; found = true; break; }
          if (!found) cand.push_back(Cand{c, 1});
        }
      }
    };
    if (new_cols(seed) > dcap || rowptr[seed + 1] - rowptr[seed] > nzcap) return 1e9;
    add(seed);
    while ((int)members.size() < tmax && !cand.empty()) {
      size_t best = 0;
      for (size_t q = 1; q < cand.size(); ++q) if (cand[q].cnt > cand[best].cnt) best = q;
      const int32_t v = cand[best].node;
      cand[best] = cand.back();
      cand.pop_back();
      if (is_in(members, v)) continue;
      if ((int)seen.size() + new_cols(v) > dcap || nz + rowptr[v + 1] - rowptr[v] > nzcap) continue;
      add(v);
    }
    rows += (int64_t)members.size();
    cols += (int64_t)seen.size();
  }
  return rows > 0 ? (double)cols / (double)rows : 1e9;
}

// Tile lists of the STORED CSR: per tile the distinct indices of its rows and their columns (ascending unless SLQ_RING_ORDER
// says otherwise), per nonzero the position of its column in that list, per row the position of the row itself.
inline void build_tile_meta(int64_t n, const int32_t *rowptr, const int32_t *colind, const std::vector<int32_t> &tile_row,
                            std::vector<int32_t> &tile_ptr, std::vector<int32_t> &tile_cols, std::vector<int32_t> &lcol,
                            std::vector<int32_t> &self_idx, int *max_cols, const OperatorSwitches &osw) {
  const size_t ntiles = tile_row.size() - 1;
  tile_ptr.assign(ntiles + 1, 0);
  tile_cols.clear();
  lcol.assign((size_t)rowptr[n] + kCsrPad, 0);
  self_idx.assign((size_t)n, 0);
  const int line_order = osw.ring_order;
  const int pieces = host_threads();
  std::vector<std::vector<int32_t>> local((size_t)pieces);  // every piece's lists, in tile order
  std::vector<int> mx_piece((size_t)pieces, 0);
  const bool ok = parallel_pieces(pieces, (int64_t)ntiles, [&](int piece, int64_t t0, int64_t t1) {
    std::vector<int32_t> u, pos, ordered;
    std::vector<int32_t> &mine = local[(size_t)piece];
    int mx = 0;
    for (int64_t t = t0; t < t1; ++t) {
      const int64_t r0 = tile_row[(size_t)t], r1 = tile_row[(size_t)t + 1];
      u.clear();
      for (int64_t r = r0; r < r1; ++r) {
        u.push_back((int32_t)r);
        for (int32_t p = rowptr[r]; p < rowptr[r + 1]; ++p) u.push_back(colind[p]);
      }
      std::sort(u.begin(), u.end());
      u.erase(std::unique(u.begin(), u.end()), u.end());
      mx = std::max(mx, (int)u.size());
      // position of every distinct index in the tile's list = the order its panel rows are landed in. Ascending by default;
      // line_order 1: the tile's own rows first, then the rows below them, then the rows above (experiments, SLQ_RING_ORDER)
      pos.resize(u.size());
      if (line_order == 0) {
        for (size_t q = 0; q < u.size(); ++q) pos[q] = (int32_t)q;
      } else {
        const size_t lo = (size_t)(std::lower_bound(u.begin(), u.end(), (int32_t)r0) - u.begin());
        const size_t own = (size_t)(r1 - r0);
        for (size_t q = 0; q < u.size(); ++q) pos[q] = (int32_t)(q < lo ? own + q : (q < lo + own ? q - lo : q));
      }
      ordered.resize(u.size());
      for (size_t q = 0; q < u.size(); ++q) ordered[(size_t)pos[q]] = u[q];
      for (int64_t r = r0; r < r1; ++r) {
        self_idx[(size_t)r] = pos[(size_t)(std::lower_bound(u.begin(), u.end(), (int32_t)r) - u.begin())];
        for (int32_t p = rowptr[r]; p < rowptr[r + 1]; ++p)
          lcol[(size_t)p] = pos[(size_t)(std::lower_bound(u.begin(), u.end(), colind[p]) - u.begin())];
      }
      mine.insert(mine.end(), ordered.begin(), ordered.end());
      tile_ptr[(size_t)t + 1] = (int32_t)ordered.size();  // (the list's length for now; offsets below)
    }
    mx_piece[(size_t)piece] = mx;
  });
  if (!ok) throw std::bad_alloc();
  for (size_t t = 0; t < ntiles; ++t) tile_ptr[t + 1] += tile_ptr[t];
  tile_cols.reserve((size_t)tile_ptr[ntiles] + kCsrPad);
  for (auto &v : local) tile_cols.insert(tile_cols.end(), v.begin(), v.end());
  tile_cols.insert(tile_cols.end(), kCsrPad, 0);
  *max_cols = *std::max_element(mx_piece.begin(), mx_piece.end());
}

// What the ring-fed passes read (SLQ_TILES=2; layouts in slq_kernels.hpp / slq_ring.hpp): per tile a descriptor of R blocks
// of 64 words and a record of its CSR in the tile's own numbering, every record at a 16-byte boundary of one blob that ends
// in a spare record's worth of zeros (a record is fetched in whole KiB). R = 1: the tiles as clustered (k_csr_ring_pass and
// k_ring_pass<LPR = 64>); R = 2, 4: tiles of R merged base tiles for panels of 64 / R lanes per row - block b of the
// descriptor lists the lines b, R + b, 2R + b, ... (the lines lane group b lands), the last one repeated to the end of its DMA.
template <typename F>
inline void build_ring_stream(int R, const int32_t *rowptr, const F *vals, const std::vector<int32_t> &tile_row, const std::vector<int32_t> &tile_ptr,
                              const std::vector<int32_t> &tile_cols, const std::vector<int32_t> &lcol, const std::vector<int32_t> &self_idx,
                              RawBuf<int32_t> &desc, RawBuf<char> &rec, bool *pad_rows = nullptr) {
  const size_t ntiles = tile_row.size() - 1;
  const size_t dw = (size_t)64 * R, head_bytes = (size_t)kRecHeadBytes * R;
  const int valoff_w = 16 * R - 1, self_w = 16 * R;
  desc.alloc(ntiles * dw);  // (zeroed tile by tile below, by the thread that fills the tile)
  // *pad_rows (the alpha-only pass's upper-triangle streams): every row's entries padded to a multiple of four, at least four, with
  // {the row's own line, 0} - its consumer then reads a row's entries four at a time with aligned 16-byte LDS reads and
  // without a single per-entry condition (slq_ring.hpp: do_alpha_padded). Given up (*pad_rows = false) if some tile's record
  // would outgrow its slot.
  bool pad = pad_rows && *pad_rows;
  auto padded = [](int32_t cnt) { return std::max<int32_t>(4, (cnt + 3) / 4 * 4); };
  if (pad) {
    for (size_t t = 0; t < ntiles && pad; ++t) {
      size_t e = 0;
      for (int32_t r = tile_row[t]; r < tile_row[t + 1]; ++r) e += (size_t)padded(rowptr[r + 1] - rowptr[r]);
      if (head_bytes + e * (4 + sizeof(F)) > (size_t)((kRingRecStride * R + 1023) / 1024 * 1024)) pad = false;
    }
  }
  if (pad_rows) *pad_rows = pad;
  // where every record starts (its size follows from the tile's entry count alone), then the tiles in parallel
  std::vector<size_t> off(ntiles + 1, 0);
  for (size_t t = 0; t < ntiles; ++t) {
    const int32_t r0 = tile_row[t];
    size_t nz = (size_t)(rowptr[tile_row[t + 1]] - rowptr[r0]);
    if (pad) {
      nz = 0;
      for (int32_t r = r0; r < tile_row[t + 1]; ++r) nz += (size_t)padded(rowptr[r + 1] - rowptr[r]);
    }
    const size_t nzp = (nz + 3) / 4 * 4;
    off[t + 1] = off[t] + (head_bytes + nzp * 4 + nzp * sizeof(F) + 15) / 16 * 16;
  }
  rec.alloc(off[ntiles] + (size_t)kRingMetaBytes * R);
  memset(rec.data() + off[ntiles], 0, (size_t)kRingMetaBytes * R);  // the spare record behind the last one
  const bool ok = parallel_pieces(host_threads(), (int64_t)ntiles, [&](int, int64_t t0, int64_t t1) {
    for (int64_t tt = t0; tt < t1; ++tt) {
      const size_t t = (size_t)tt;
      const int32_t r0 = tile_row[t], rows = tile_row[t + 1] - r0, p0 = rowptr[r0];
      int32_t nz = rowptr[r0 + rows] - p0;
      if (pad) {
        nz = 0;
        for (int32_t i = 0; i < rows; ++i) nz += padded(rowptr[r0 + i + 1] - rowptr[r0 + i]);
      }
      const int32_t D = tile_ptr[t + 1] - tile_ptr[t];
      const size_t nzp = ((size_t)nz + 3) / 4 * 4, valoff = head_bytes + nzp * 4, bytes = off[t + 1] - off[t];
      memset(rec.data() + off[t], 0, bytes);
      memset(desc.data() + t * dw, 0, dw * 4);
      int32_t *head = (int32_t *)(rec.data() + off[t]);
      head[valoff_w] = (int32_t)valoff;
      for (int32_t i = 0; i < rows; ++i) head[self_w + i] = self_idx[(size_t)(r0 + i)];
      if (!pad) {
        for (int32_t i = 0; i <= rows; ++i) head[i] = rowptr[r0 + i] - p0;
        memcpy(rec.data() + off[t] + head_bytes, lcol.data() + p0, (size_t)nz * 4);
        memcpy(rec.data() + off[t] + valoff, vals + p0, (size_t)nz * sizeof(F));
      } else {
        int32_t *lc_out = (int32_t *)(rec.data() + off[t] + head_bytes);
        F *va_out = (F *)(rec.data() + off[t] + valoff);
        int32_t w = 0;
        for (int32_t i = 0; i < rows; ++i) {
          const int32_t q0 = rowptr[r0 + i], cnt = rowptr[r0 + i + 1] - q0, pc = padded(cnt);
          head[i] = w;
          for (int32_t q = 0; q < pc; ++q) {
            lc_out[w + q] = q < cnt ? lcol[(size_t)(q0 + q)] : self_idx[(size_t)(r0 + i)];
            va_out[w + q] = q < cnt ? vals[q0 + q] : (F)0;
          }
          w += pc;
        }
        head[rows] = w;
      }
      int32_t *d = desc.data() + t * dw;
      d[kDescCols] = D;
      d[kDescRecOff] = (int32_t)(off[t] / 16);
      d[kDescRecChunks] = (int32_t)((bytes + 1023) / 1024);
      d[kDescRow0] = r0;
      d[kDescRows] = rows;
      const int32_t nd = (D + R - 1) / R;
      if (R == 1) {  // (de-interleaved: even lines, then odd ones - slq_common.hpp: ring1_list_pos)
        for (int32_t c = 0; c < D; ++c) d[kDescList + ring1_list_pos(c)] = tile_cols[(size_t)tile_ptr[t] + c];
      } else {
        for (int32_t c = 0; c < nd * R; ++c) d[(size_t)(c % R) * 64 + kDescList + c / R] = tile_cols[(size_t)tile_ptr[t] + std::min(c, D - 1)];
      }
    }
  });
  if (!ok) throw std::bad_alloc();
}

// Tiles of the upper-triangle stream (the alpha-only pass, r04). That pass lands 31-32 GB/s per CU by LDS-DMA whatever the operator (configs[1]: 1.64 KiB per row,
// 0.40 ms; 100^3: 2.65 KiB per row, 0.65 ms) - the DMA path's own cadence - so what shortens it is fewer landed lines per row. The base tiles are cut to what a slot
// holds of FULL rows; over the upper triangle the same rows need two thirds of the lines, so consecutive base tiles of a chunk - neighbours in the sweep, which share
// halo - are joined while the run keeps to kRingTileRows rows, kRingTileCols distinct lines (rows and upper columns) and kRingTileNnz padded entries: 100^3, 118,940 ->
// 107,848 tiles, alpha pass 0.652 -> 0.607 ms. (Cutting the chunk's rows anew, row by row, to the same caps gives 12.9-row tiles that straddle cluster boundaries and
// land MORE lines per row, 2.65 against 2.47: 0.82 ms. Not kept.) Tiles stay contiguous row ranges of one XCD chunk; kernel and stream format do not change.
// each_upper(r, consider): calls consider(c) for every column c >= r of stored row r and returns how many there were (the upper
// triangle's CSR, or - before that exists - the caller's CSR seen through the permutation: the columns' order does not matter)
template <typename EachUpper>
inline void regroup_upper_tiles_impl(EachUpper each_upper, const std::vector<int32_t> &tile_row, const int32_t xcd_tile[9],
                                     std::vector<int32_t> &tile_row_u, int32_t xcd_tile_u[9]) {
  auto padded = [](int32_t cnt) { return std::max<int32_t>(4, (cnt + 3) / 4 * 4); };
  // every chunk on its own (in parallel): consecutive base tiles - neighbours in the sweep - joined while the run keeps to the caps
  std::vector<int32_t> cuts[8];
  const bool ok = parallel_pieces(8, 8, [&](int, int64_t x0, int64_t x1) {
    for (int64_t x = x0; x < x1; ++x) {
      std::vector<int32_t> &out = cuts[x];
      if (xcd_tile[x] >= xcd_tile[x + 1]) continue;
      // membership by stamps (r04: the lists were searched linearly - 25 ms of a 100^3 operator's creation): in_run[c - base] == run: c is a line of
      // the current run; in_tile[c - base] == stamp: c was counted for the base tile under consideration. Every column of a chunk's rows is >= base.
      const int32_t base = tile_row[(size_t)xcd_tile[x]], n_all = tile_row.back();
      std::vector<int32_t> in_run((size_t)(n_all - base), -1), in_tile((size_t)(n_all - base), -1);
      int32_t run = 0, stamp = 0;
      int nl = 0, rows = 0, nz = 0;
      for (int32_t t = xcd_tile[x]; t < xcd_tile[x + 1]; ++t) {
        const int32_t r0 = tile_row[(size_t)t], r1 = tile_row[(size_t)t + 1];
        // what this base tile lists - its rows and their upper columns, each once - and how much of that the run does not list yet
        int32_t all[kRingTileCols + 16];
        int na = 0, nf = 0;
        int32_t pz = 0;
        auto consider = [&](int32_t c) {
          const size_t k = (size_t)(c - base);
          if (in_tile[k] == stamp) return;
          in_tile[k] = stamp;
          if (na < kRingTileCols + 16) all[na++] = c, nf += in_run[k] != run;
        };
        for (int32_t r = r0; r < r1; ++r) {
          consider(r);
          pz += padded(each_upper(r, consider));
        }
        ++stamp;
        if (rows > 0 && (rows + (r1 - r0) > kRingTileRows || nl + nf > kRingTileCols || nz + pz > kRingTileNnz)) {
          nl = rows = nz = 0;  // cut: this base tile opens the next run (its own lines: everything it lists)
          ++run;
        }
        if (rows == 0) out.push_back(r0);
        for (int q = 0; q < na && nl < 2 * kRingTileCols + 16; ++q) {
          int32_t &m = in_run[(size_t)(all[q] - base)];
          if (m != run) m = run, ++nl;
        }
        rows += r1 - r0;
        nz += pz;
      }
    }
  });
  if (!ok) throw std::bad_alloc();
  tile_row_u.clear();
  for (int x = 0; x < 8; ++x) {
    xcd_tile_u[x] = (int32_t)tile_row_u.size();
    tile_row_u.insert(tile_row_u.end(), cuts[x].begin(), cuts[x].end());
  }
  xcd_tile_u[8] = (int32_t)tile_row_u.size();
  tile_row_u.push_back(tile_row.back());
}
inline void regroup_upper_tiles(const int32_t *urp, const int32_t *uci, const std::vector<int32_t> &tile_row, const int32_t xcd_tile[9],
                                std::vector<int32_t> &tile_row_u, int32_t xcd_tile_u[9]) {
  regroup_upper_tiles_impl(
      [&](int32_t r, auto &consider) {
        for (int32_t q = urp[r]; q < urp[r + 1]; ++q) consider(uci[q]);
        return urp[r + 1] - urp[r];
      },
      tile_row, xcd_tile, tile_row_u, xcd_tile_u);
}

// If the CSR (rows sorted, no duplicates) is exactly symmetric, emit its upper triangle with the strict
// upper entries doubled and return true. Row ranges in parallel: every off-diagonal entry (i, j) looks its mirror (j, i)
// up by bisection in row j (rows are sorted - checked on the way) and compares the values; the upper entries are then
// counted per row, placed by a prefix sum and written, again by row ranges.
template <typename F>
inline bool build_symmetric_upper(int64_t n, const int32_t *rowptr, const int32_t *colind, const F *vals,
                                  std::vector<int32_t> &urp, std::vector<int32_t> &uci, std::vector<char> &uva) {
  urp.assign((size_t)n + 1, 0);
  const int pieces = host_threads();
  std::vector<char> bad((size_t)pieces, 0);
  if (!parallel_pieces(pieces, n, [&](int piece, int64_t i0, int64_t i1) {
        for (int64_t i = i0; i < i1 && !bad[(size_t)piece]; ++i) {
          int32_t up = 0;
          for (int32_t q = rowptr[i]; q < rowptr[i + 1]; ++q) {
            const int32_t j = colind[q];
            if (q > rowptr[i] && colind[q - 1] >= j) { bad[(size_t)piece] = 1; break; }  // unsorted or duplicate
            up += j >= i;
            if (j == i) continue;
            const int32_t *lo = colind + rowptr[j], *hi = colind + rowptr[j + 1];
            const int32_t *m = std::lower_bound(lo, hi, (int32_t)i);
            if (m == hi || *m != (int32_t)i || !(vals[m - colind] == vals[q])) { bad[(size_t)piece] = 1; break; }
          }
          urp[(size_t)i + 1] = up;
        }
      }))
    return false;
  if (std::any_of(bad.begin(), bad.end(), [](char c) { return c != 0; })) return false;
  for (int64_t i = 0; i < n; ++i) urp[(size_t)i + 1] += urp[(size_t)i];
  const size_t nu = (size_t)urp[(size_t)n];
  uci.resize(nu);
  uva.resize(nu * sizeof(F));
  F *uv = (F *)uva.data();
  return parallel_pieces(pieces, n, [&](int, int64_t i0, int64_t i1) {
    for (int64_t i = i0; i < i1; ++i) {
      size_t w = (size_t)urp[(size_t)i];
      for (int32_t q = rowptr[i]; q < rowptr[i + 1]; ++q) {
        const int32_t j = colind[q];
        if (j < i) continue;
        uci[w] = j;
        uv[w] = j == i ? vals[q] : (F)2 * vals[q];
        ++w;
      }
    }
  });
}
// The same over the caller's CSR seen through the permutation (stored row r = caller row perm[r], caller row c is stored row
// inv[c]): what the device-side build regroups while the stored CSR and its upper triangle are still being built on the device.
// The columns' order does not matter, so the result is that of regroup_upper_tiles on the stored upper triangle.
inline void regroup_upper_tiles_permuted(const int32_t *rowptr, const int32_t *colind, const std::vector<int32_t> &perm, const std::vector<int32_t> &inv,
                                         const std::vector<int32_t> &tile_row, const int32_t xcd_tile[9], std::vector<int32_t> &tile_row_u, int32_t xcd_tile_u[9]) {
  regroup_upper_tiles_impl(
      [&](int32_t r, auto &consider) {
        const int32_t o = perm[(size_t)r];
        int32_t cnt = 0;
        for (int32_t q = rowptr[o]; q < rowptr[o + 1]; ++q) {
          const int32_t c = inv[(size_t)colind[q]];
          if (c >= r) consider(c), ++cnt;
        }
        return cnt;
      },
      tile_row, xcd_tile, tile_row_u, xcd_tile_u);
}
// Whether the upper-triangle stream gets tiles of its own (runs of the base tiles) or keeps the base tiles: not where those are
// as tall as a tile gets - a 5-point grid's 13.9 of 14 rows: nothing to join, 10-20 ms of host time saved. Both storage builders ask here.
inline bool regroup_upper_wanted(const OperatorSwitches &osw, int64_t n, size_t ntiles) {
  const bool tall_already = (double)n / (double)ntiles > 0.8 * kRingTileRows;
  return osw.ring_upper_regroup != 0 && !tall_already;
}

// ---------------------------------------------------------------------------------------------------
// the layout of a CSR operator, as a value
// ---------------------------------------------------------------------------------------------------
struct CsrView {  // the caller's CSR (validated: slq.hip)
  int64_t n, nnz;
  const int32_t *rowptr, *colind;
};
// What must be known before the caller's CSR may start its way to the device (the early upload of the device-side build).
struct LayoutPrefilter {
  int reorder_mode;       // SLQ_REORDER as this creation takes it (0 for plain operators)
  int tmode;              // SLQ_TILES likewise
  bool try_tiles;         // the operator is large enough for tiles and the sample did not turn it away
  double sample_quality;  // distinct panel rows per row of the 256-cluster sample (-1: not taken)
};
struct OperatorLayout {
  std::vector<int32_t> perm, inv;      // stored row i = caller row perm[i], caller row r = stored row inv[r]; empty: the caller's order. inv is computed once, here
  std::vector<int32_t> rowptr_stored;  // the row pointer of the stored (permuted) CSR, computed once, here; empty with perm
  std::vector<int32_t> tile_row;       // [ntiles + 1] first stored row of every tile (empty: no tiles)
  int32_t xcd_tile[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  bool have_tiles = false;
  double rms_dist = -1.0;              // rms |i - j| over the stored nonzeros inside an XCD chunk (-1: no nonzeros)
};

inline std::vector<int32_t> inverse_permutation(const std::vector<int32_t> &perm) {
  std::vector<int32_t> inv(perm.size());
  for (size_t i = 0; i < perm.size(); ++i) inv[(size_t)perm[i]] = (int32_t)i;
  return inv;
}

// rms index distance of the nonzeros whose two ends lie in the same XCD chunk (links that cross
// chunks are served by another XCD's L2 whatever the order inside the chunks); inv: caller row -> stored row (null: identity)
inline double mean_dist(const CsrView &A, const std::vector<int32_t> *inv) {
  const int64_t n = A.n, rchunk = (n + 7) / 8;
  const int32_t *rowptr = A.rowptr, *colind = A.colind;
  const int pieces = 8;  // (a fixed partition: the sum does not depend on how many threads ran it)
  std::vector<double> acc((size_t)pieces, 0.0);
  std::vector<int64_t> cnt((size_t)pieces, 0);
  if (!parallel_pieces(pieces, n, [&](int piece, int64_t i0, int64_t i1) {
    double a = 0.0;
    int64_t c = 0;
    for (int64_t i = i0; i < i1; ++i) {
      const int64_t ii = inv ? (*inv)[(size_t)i] : i;
      for (int32_t q = rowptr[i]; q < rowptr[i + 1]; ++q) {
        if (colind[q] / rchunk != i / rchunk) continue;
        const int64_t jj = inv ? (*inv)[(size_t)colind[q]] : colind[q];
        const double dd = (double)(ii > jj ? ii - jj : jj - ii);
        a += dd * dd;
        ++c;
      }
    }
    acc[(size_t)piece] = a;
    cnt[(size_t)piece] = c;
  })) throw std::bad_alloc();
  double a = 0.0;
  int64_t c = 0;
  for (int t = 0; t < pieces; ++t) a += acc[(size_t)t], c += cnt[(size_t)t];  // (piece order: the same value whatever the timing)
  return std::sqrt(a / (double)std::max<int64_t>(c, 1));
}

// SLQ_REORDER: 0 never, 1 operators with n >= 65536, 2 always, unset = automatic. Measured (DESIGN.md
// §5.3): on the 2-D grid of configs[1] (rms |i-j| of the nonzeros = 632 rows) it RAISED the alpha pass's
// fetch traffic from 6.5 to 8.9 GB and the step time by 10 %; on 3-D grids (100^3: rms |i-j| = 5345,
// 126^3: 8486) whose natural-order halo no longer fits any cache level it is 9-12 % FASTER. Automatic
// mode therefore reorders only when the rms index distance exceeds 2048 rows AND the permutation cuts
// it to 60 % or less (random graphs gain nothing and are left alone).
// Workgroup tiles (SLQ_TILES): the rows are regrouped into compact clusters = the tiles of k_csr_tile_pass /
// k_csr_ring_pass, on top of a base order. Kept only if the tiles actually share rows: at most kTileMaxColsPerRow distinct
// panel rows per tile row (5-point grid: 2.1, 7-point grid: 3.9 with the ring kernel's 36-row images, random graph: 10+).
// Unasked (SLQ_TILES unset) only operators of 65536 rows and more are tried - below that a pass is launch-bound anyway.
// plain: rows stay in the caller's order and there are no tiles (operators whose values change after creation).
inline LayoutPrefilter layout_prefilter(const CsrView &A, const OperatorSwitches &osw, bool plain) {
  LayoutPrefilter pre;
  pre.reorder_mode = plain ? 0 : osw.reorder;
  pre.tmode = plain ? 0 : osw.tiles;
  pre.try_tiles = pre.tmode != 0 && A.nnz > 0 && A.n >= (osw.tiles_forced ? 4096 : 65536);
  pre.sample_quality = -1.0;
  if (pre.try_tiles) {
    // (a sample cluster grows on the caller's numbering, the real ones on the reordered chunk: 4.3 against 3.9 on a 7-point grid,
    // 2.3 against 2.1 on a 5-point one, 12-16 on the operators this is meant to turn away. 25 % of margin keeps it a filter for
    // those only)
    const bool ringed = pre.tmode == 2;
    const double q = sample_tile_quality(A.n, A.rowptr, A.colind, ringed ? kRingTileRows : std::max(1, std::min(osw.tile_rows, 64)),
                                         ringed ? kRingTileCols : std::max(8, std::min(osw.tile_cols, kTileCols)),
                                         ringed ? kRingTileNnz : std::numeric_limits<int>::max());
    if (osw.debug != 0) fprintf(stderr, "[slq] tiles: sample of 256 clusters: %.2f distinct panel rows per row\n", q);
    pre.sample_quality = q;
    if (q > 1.25 * kTileMaxColsPerRow) pre.try_tiles = false;
  }
  return pre;
}

// clusters on top of `base` (stored row -> caller row, with its inverse; null: the caller's order): L's tiles, and on success
// `order`, the new order. False: no tiling, or tiles that share too little
inline bool cluster_tiles(const CsrView &A, const OperatorSwitches &osw, const std::vector<int32_t> *base, const std::vector<int32_t> *base_inv,
                          OperatorLayout &L, std::vector<int32_t> &order, PhaseClock *clk) {
  int64_t dsum = 0;  // distinct indices (rows and columns) summed over the tiles: the clusters count them as they grow
  if (!build_clusters(A.n, A.rowptr, A.colind, base ? base->data() : nullptr, base ? base_inv->data() : nullptr, order, L.tile_row, L.xcd_tile, osw, &dsum)) return false;
  if (clk) clk->lap("  clusters");
  const double per_row = (double)dsum / (double)A.n;
  if (osw.debug != 0)
    fprintf(stderr, "[slq] tiles: %zu clusters, %.2f rows each, %.2f distinct panel rows per row (limit %.1f)\n", L.tile_row.size() - 1,
            (double)A.n / (double)(L.tile_row.size() - 1), per_row, kTileMaxColsPerRow);
  return per_row <= kTileMaxColsPerRow;
}

// The row order and the tiles of an operator that passed layout_prefilter. clk (or null): the phases' laps (SLQ_DEBUG).
inline OperatorLayout decide_layout(const CsrView &A, const OperatorSwitches &osw, const LayoutPrefilter &pre, PhaseClock *clk) {
  OperatorLayout L;
  const int64_t n = A.n, nnz = A.nnz;
  const int reorder_mode = pre.reorder_mode, tmode = pre.tmode;
  const bool try_tiles = pre.try_tiles;
  auto adopt = [&](std::vector<int32_t> &order) {
    L.perm.swap(order);
    L.inv = inverse_permutation(L.perm);
  };
  std::vector<int32_t> rcm_perm;  // the in-chunk Cuthill-McKee order, computed at most once
  const int sub_env = osw.rcm_sub;  // 0: 1 piece, except for the tile sweep below
  auto rcm_order = [&]() -> const std::vector<int32_t> & {
    if (rcm_perm.empty()) xcd_rcm_permutation(n, A.rowptr, A.colind, rcm_perm, std::max(1, sub_env), nullptr);
    return rcm_perm;
  };
  // Ring-fed tiles sweep a chunk tile after tile, 32 CUs abreast, and re-read a neighbour tile's rows from L2 only if the
  // neighbour is at most a few dozen tiles away: the BASE order must have short level sets, whatever the index distances
  // are. On the 2-D grid of configs[1] in its natural order (grid rows of 1000 = 270 tiles) every vertical neighbour was
  // fetched again (7.5 GB per dots pass against 6.3 algorithmic); on the in-chunk Cuthill-McKee order (levels of <= 125
  // nodes = 34 tiles) the pass fetches 6.37 GB. So mode 2 clusters the Cuthill-McKee order unless SLQ_REORDER=0 forbids it.
  // ... and level sets no longer than about one round of the sweep (32 CUs x 10 rows): a 12.5-plane slab of a 100^3 grid has
  // level sets of 590 rows on average - its tiles then fetch 8.7 GB per dots pass against 6.1 algorithmic - so the chunk's
  // order is cut into 4, 16, 64 runs of levels, each reordered on its own (xcd_rcm_permutation), until they are: 16 pieces
  // there (level sets of ~200 rows, 7.5 GB). SLQ_RCM_SUB fixes the number of pieces.
  if (try_tiles && tmode == 2 && reorder_mode != 0) {
    if (sub_env <= 0) {
      double w = 0.0;
      std::vector<int32_t> level1;  // the chunks' own order (k = 1), which every finer attempt starts from
      for (int k = 1; k <= 64; k *= 4) {
        if (k == 4) level1 = rcm_perm;
        xcd_rcm_permutation(n, A.rowptr, A.colind, rcm_perm, k, &w, k > 1 ? &level1 : nullptr);
        if (clk) clk->lap("  Cuthill-McKee in the chunks");
        if (osw.debug != 0) fprintf(stderr, "[slq] tiles: %d piece(s) per chunk: level sets of %.0f rows on average\n", k, w);
        if (w <= kTileLevelRows) break;
      }
    }
    std::vector<int32_t> order;
    const std::vector<int32_t> base_inv = inverse_permutation(rcm_order());  // (of the base order, which the clusters then replace)
    if (cluster_tiles(A, osw, &rcm_perm, &base_inv, L, order, clk)) {
      L.have_tiles = true;
      adopt(order);
    } else if (sub_env <= 0) {
      rcm_perm.clear();  // declined: the generic passes keep their own (one-piece) order, decided below
    }
  }
  if (clk) clk->lap("base order + clusters");
  bool want = false;
  if (nnz > 0 && !L.have_tiles) {
    if (reorder_mode == 2) want = true;
    else if (reorder_mode == 1) want = n >= 65536;
    else if (reorder_mode < 0) want = n >= 65536 && mean_dist(A, nullptr) > 2048.0;
  }
  if (want) {
    std::vector<int32_t> order = rcm_order();
    adopt(order);
    const double d_new = mean_dist(A, &L.inv);
    if (reorder_mode < 0 && d_new > 0.6 * mean_dist(A, nullptr)) {
      L.perm.clear();  // no locality to gain: keep the caller's order
      L.inv.clear();
    } else {
      L.rms_dist = d_new;
    }
  }
  // tiles on top of whatever order was chosen above: mode 1, and mode 2 when SLQ_REORDER=0 kept it from its own base order
  if (try_tiles && !L.have_tiles && (tmode == 1 || reorder_mode == 0)) {
    std::vector<int32_t> order;
    const bool based = !L.perm.empty();
    if (cluster_tiles(A, osw, based ? &L.perm : nullptr, based ? &L.inv : nullptr, L, order, clk)) {
      L.have_tiles = true;
      adopt(order);
    }
  }
  if (L.have_tiles) L.rms_dist = mean_dist(A, &L.inv);
  if (L.rms_dist < 0.0 && nnz > 0) L.rms_dist = mean_dist(A, nullptr);
  if (!L.have_tiles) {  // (what a declined attempt left behind)
    L.tile_row.clear();
    for (int x = 0; x < 9; ++x) L.xcd_tile[x] = 0;
  }
  if (!L.perm.empty()) {
    L.rowptr_stored.resize((size_t)n + 1);
    L.rowptr_stored[0] = 0;
    for (int64_t i = 0; i < n; ++i) {
      const int32_t o = L.perm[(size_t)i];
      L.rowptr_stored[(size_t)i + 1] = L.rowptr_stored[(size_t)i] + (A.rowptr[o + 1] - A.rowptr[o]);
    }
  }
  if (clk) clk->lap("reorder decision");
  return L;
}

}  // namespace slq
