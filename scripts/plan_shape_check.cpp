// plan_shape_check.cpp — plan_shape() of csrc/slq_plan_shape.hpp over the FULL product of the operators, requests and switches
// whose three sub-products tests/test_plan_shape_cpu.py covers (tests/_plan_cases.py builds them by the same rules), with the
// invariants the kernels rely on checked on every answer. A stand-alone host program for the sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I primate_amd/csrc scripts/plan_shape_check.cpp -o plan_shape_check
//   ./plan_shape_check
// It includes nothing but the header under test; no device, no library.
#include "slq_plan_shape.hpp"

#include <cstdio>
#include <vector>

using namespace slq;

static long g_cases = 0, g_failed = 0;
#define CHECK(cond)                                                                 \
  do {                                                                              \
    if (!(cond)) {                                                                  \
      if (g_failed++ < 20) fprintf(stderr, "case %ld: %s failed\n", g_cases, #cond); \
    }                                                                               \
  } while (0)

static void fill_xcd(int32_t *t, int per_xcd) {
  for (int x = 0; x < 9; ++x) t[x] = x * per_xcd;
}

// the operators of the grid (tests/_plan_cases.py: OPERATORS)
static std::vector<PlanFacts> operators() {
  std::vector<PlanFacts> ops;
  const int64_t n2 = 96 * 96, n3 = 20 * 20 * 20;
  const int64_t nnz5 = 5 * n2 - 4 * 96, nnz7 = 7 * n3 - 6 * 400;
  auto csr = [](int64_t n, int64_t nnz, bool upper) {
    PlanFacts f;
    f.kind = OP_CSR, f.n = n, f.nnz = nnz, f.upper = upper, f.nnz_u = upper ? (nnz + n) / 2 : 0;
    return f;
  };
  ops.push_back(csr(n2, nnz5, true));    // no tiles; nnz / n < 5.5, upper gathers < 3.2
  ops.push_back(csr(n2, nnz5, false));   // ... full rows: gathers > 3.2
  ops.push_back(csr(n3, nnz7, true));    // nnz / n > 5.5 (pipelined), upper gathers > 3.2
  {
    PlanFacts f = csr(n2, nnz5, true);
    f.far_per_row = 6.0;                 // gathers not served from cache
    ops.push_back(f);
    f = csr(n2, nnz5, true);
    f.affine = 1;
    ops.push_back(f);
  }
  for (int per_xcd : {48, 3}) {          // barrier tiles
    PlanFacts f = csr(n2, nnz5, true);
    f.has_tiles = 1, f.tiles_max_cols = 72;
    fill_xcd(f.xcd_tile, per_xcd);
    ops.push_back(f);
  }
  for (int upper_stream = 0; upper_stream < 2; ++upper_stream)
    for (double upr : {2.0, 3.0})        // both sides of SLQ_RING_ALPHA_MAX_X100 / 100 = 2.6
      for (int merged = 0; merged < 2; ++merged)
        for (int per_xcd : {83, 2}) {
          if (!upper_stream && upr != 2.0) continue;
          PlanFacts f = csr(n2, nnz5, true);
          f.has_tiles = 1, f.tiles_ringed = 1, f.tiles_max_cols = 36;
          fill_xcd(f.xcd_tile, per_xcd);
          f.upper_stream = upper_stream, f.upper_padded = upper_stream, f.upper_per_row = upper_stream ? upr : 0.0;
          if (upper_stream) fill_xcd(f.xcd_tile_u, (per_xcd + 1) / 2);
          for (int i = 0; i < 2 && merged; ++i) {
            f.merged[i].available = 1, f.merged[i].upper = upper_stream, f.merged[i].u_padded = upper_stream;
            fill_xcd(f.merged[i].xcd_tile, (per_xcd + (2 << i) - 1) / (2 << i));
          }
          ops.push_back(f);
        }
  for (int64_t lda : {300, 301}) {       // dense, even and odd lda
    PlanFacts f;
    f.kind = OP_DENSE, f.n = 300, f.nnz = 300 * 300, f.lda = lda;
    ops.push_back(f);
  }
  {
    PlanFacts f;
    f.kind = OP_DENSE, f.n = 5000, f.nnz = 5000 * 5000, f.lda = 5000;
    ops.push_back(f);
    f = PlanFacts();
    f.kind = OP_GRAM, f.n = 200, f.mrows = 350, f.nnz = 1400;
    ops.push_back(f);
    f = PlanFacts();
    f.kind = OP_CALLBACK, f.n = 500;
    ops.push_back(f);
  }
  return ops;
}

static void check(const PlanFacts &f, const PlanSwitches &sw) {
  ++g_cases;
  const PlanShape s = plan_shape(f, sw);
  const size_t esz = esize_of(f.dtype);
  for (int g : {s.nblkA, s.nblkU, s.nblkF, s.nblkT}) CHECK(g > 0 && g % 8 == 0);
  CHECK(s.nblkS > 0);
  if (f.has_tiles) {
    int mn = 1 << 30;
    for (int x = 0; x < 8; ++x) mn = std::min(mn, std::max(1, s.rs_xcd[x + 1] - s.rs_xcd[x]));
    CHECK(s.nblkT / 8 <= mn);
  }
  CHECK(s.part_maxblk == std::max({s.nblkA, s.nblkS, s.nblkU, s.nblkF, s.nblkT}));
  CHECK(s.bpad == s.NP * s.PW && s.bpad >= f.nprobes && s.bpad - s.PW < f.nprobes);
  CHECK(s.LPR == 8 || s.LPR == 16 || s.LPR == 32 || s.LPR == 64);
  const ScalOffsets &o = s.scal;
  const size_t offs[] = {o.alpha, o.nu_margin, o.nu, o.vnorm2, o.coefA, o.coefB, o.cross, o.gram, o.gamma, o.end};
  CHECK(offs[0] == 0);
  for (int i = 0; i + 1 < 10; ++i) CHECK(offs[i] < offs[i + 1] || (i == 1 && f.orth == 0));  // disjoint and ordered (the nu margin is empty at orth 0)
  CHECK(o.nu - o.nu_margin == (size_t)f.orth * s.bpad && o.end - o.gamma == (size_t)s.rmax * s.bpad);
  CHECK(o.end * 8 == s.ws[WS_SCAL].bytes);
  CHECK(s.active.steps == (size_t)s.bpad && s.active.fail == 2 * (size_t)s.bpad && s.active.ring_fail == s.active.fail + 1 && s.active.fail2 == s.active.fail + 2);
  CHECK(s.active.end * 4 == s.ws[WS_ACTIVE].bytes && s.active.fail2 < s.active.end);
  // the ring's slots, and the panels of an action behind or inside it, lie inside the ring region (a plan without an action
  // - Ring, Chebyshev - never reads v_slot / y_slot)
  const size_t slot_bytes = (size_t)s.slot_stride * esz;
  CHECK(s.S >= 2 && (size_t)s.S * slot_bytes <= s.ws[WS_RING].bytes);
  if (f.plan == PlanKind::KeepBasis || f.plan == PlanKind::Recompute || f.plan == PlanKind::ChebyshevAction)
    CHECK((size_t)(std::max(s.v_slot, s.y_slot) + 1) * slot_bytes <= s.ws[WS_RING].bytes && s.v_slot >= 0 && s.y_slot >= 0);
  if (f.plan == PlanKind::Recompute) CHECK(s.S >= s.acc_cols + 1 && s.v_slot >= s.S && s.y_slot > s.v_slot);
  // the estimate of the one-shot entries bounds the exact T
  CHECK(s.dense_ks >= 0 && s.dense_ks <= 16 && (size_t)s.t_slabs_bound * slot_bytes >= s.ws[WS_T].bytes);
  CHECK(plan_estimate_bytes(s, f) >= s.ws[WS_RING].bytes + s.ws[WS_T].bytes + s.ws[WS_T2].bytes);
  CHECK((f.kind == OP_CSR) == (s.ws[WS_T].bytes == 0) && (f.kind == OP_GRAM) == (s.ws[WS_T2].bytes != 0));
  for (int r = 0; r < kNumRegions; ++r) CHECK(s.ws[r].id == r);
  CHECK((s.stream == STREAM_NONE) == (s.ringR == 0 || !f.tiles_ringed));
  if (s.ringR > 1) CHECK(s.stream == (s.ringR == 2 ? STREAM_MERGED2 : STREAM_MERGED4) && f.merged[s.ringR == 2 ? 0 : 1].available && wants_merged_stream(f, sw) == s.ringR);
  // the arrays round-trip
  double fa[kNumPlanFacts], sa[kNumPlanShape], sb[kNumPlanShape];
  plan_facts_to_array(f, fa);
  plan_shape_to_array(s, sa);
  plan_shape_to_array(plan_shape(plan_facts_from_array(fa), sw), sb);
  for (int i = 0; i < kNumPlanShape; ++i) CHECK(sa[i] == sb[i]);
}

int main() {
  std::vector<PlanSwitches> switches(1);
  for (int lpr : {8, 16, 32, 64}) { PlanSwitches s; s.lpr = lpr; switches.push_back(s); }
  for (int pipe : {0, 1}) { PlanSwitches s; s.pipe = pipe; switches.push_back(s); }
  { PlanSwitches s; s.tiles = 0; switches.push_back(s); }
  for (int ks : {1, 7, 16}) { PlanSwitches s; s.dense_ksplit = ks; switches.push_back(s); }
  { PlanSwitches s; s.dense_tile16 = 1; switches.push_back(s); }
  { PlanSwitches s; s.dense_mfma = 0; switches.push_back(s); }
  { PlanSwitches s; s.omega = 2; switches.push_back(s); }
  const int probes[] = {1, 8, 16, 17, 32, 64, 128, 256, 257};
  for (const PlanFacts &op : operators())
    for (int dtype : {kF64, kF32})
      for (int num_cus : {256, 8})
        for (int kind = 0; kind < 5; ++kind)
          for (int nprobes : probes)
            for (int deg : {1, 8, 9, 30, 512, 16384})
              for (int oi = 0; oi < 4; ++oi)
                for (const PlanSwitches &sw : switches) {
                  PlanFacts f = op;
                  f.dtype = dtype, f.num_cus = num_cus, f.nprobes = nprobes, f.plan = (PlanKind)kind;
                  const bool cheb = is_cheb(f.plan);
                  if (deg > kMaxDeg && !cheb) continue;
                  if (cheb && oi) continue;  // (a Chebyshev plan has orth 0)
                  f.deg = cheb ? deg : (int)std::min<int64_t>(deg, f.n);
                  const int orths[4] = {0, 3, 6, f.deg};
                  f.orth = std::min(orths[oi], f.deg);
                  check(f, sw);
                }
  // a byte query's facts: nothing but dtype, n, nprobes, deg, orth and kind (the ring region must not need the rest)
  for (int kind = 0; kind < 3; ++kind) {
    PlanFacts f;
    f.dtype = kF32, f.n = (int64_t)3 << 31, f.nprobes = 100, f.deg = 40, f.orth = 5, f.plan = (PlanKind)kind;
    const PlanShape s = plan_shape(f, PlanSwitches());
    ++g_cases;
    CHECK(s.ws[WS_RING].bytes == (size_t)(kind == 0 ? 6 : (kind == 1 ? 41 : 11)) * (size_t)s.NP * (size_t)f.n * s.PW * 4);
  }
  printf("plan_shape_check: %ld cases, %ld failed checks\n", g_cases, g_failed);
  return g_failed ? 1 : 0;
}
