// slq_plan_shape.hpp — what creating a plan decides, as a value. Plain C++ (no HIP include): a pure function from the facts
// of an operator, a context and a request (PlanFacts) and the switches (PlanSwitches) to the plan's geometry, grids, tile
// stream, sequence flags and the table of its device allocations (PlanShape), so that it runs without a device
// (slq_debug_plan_shape, tests/test_plan_shape_cpu.py, scripts/plan_shape_check.cpp). slq_plan_create* (slq.hip) collects the
// facts, calls plan_shape() once and allocates what the table says; the byte queries read the same answer; slq_plan_destroy
// frees the table.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "slq_format.hpp"
#include "slq_kernelop.hpp"
#include "slq_kernelprecond.hpp"
#include "slq_sequence.hpp"
#include "slq_switches.hpp"
#include "slq_toeplitz.hpp"

namespace slq {

enum { OP_CSR = 0, OP_DENSE = 1, OP_CALLBACK = 2, OP_DEVICE_CALLBACK = 3, OP_GRAM = 4, OP_KERNEL = 5, OP_KERNEL_PRECOND = 6, OP_TOEPLITZ = 7 };
// (a preconditioned kernel operator - slq_kernelprecond.hpp - is a kernel operator between two applies of M = P^{-1/2})
inline bool is_kernel_kind(int kind) { return kind == OP_KERNEL || kind == OP_KERNEL_PRECOND; }
constexpr int kF32 = 0, kF64 = 1;  // == SLQ_F32, SLQ_F64 (include/slq.h; slq.hip asserts the equality)

// Ring: the window of the last orth vectors. KeepBasis: every vector. Recompute: the ring widened for the accumulation launches
// of the replay, stash and output panel behind it. Chebyshev: the orth-0 ring, moments instead of a Gauss rule
// (§4.12). ChebyshevAction: its ring holds the columns an accumulation launch consumes, the output panel behind it (§4.13).
enum class PlanKind { Ring = 0, KeepBasis = 1, Recompute = 2, Chebyshev = 3, ChebyshevAction = 4 };
inline bool is_cheb(PlanKind k) { return k == PlanKind::Chebyshev || k == PlanKind::ChebyshevAction; }
// what slq_plan_basis_mode answers: 0 ring only, 1 kept basis, 2 recompute (both Chebyshev kinds: 0)
inline int basis_mode_of(PlanKind k) { return k == PlanKind::KeepBasis ? 1 : (k == PlanKind::Recompute ? 2 : 0); }

// Everything creation reads from outside itself, and nothing else.
struct PlanFacts {
  // operator
  int kind = OP_CSR, dtype = kF64;
  int64_t n = 0, nnz = 0, nnz_u = 0;
  int upper = 0;            // exactly symmetric CSR: it has the upper-triangle copy (slq_operator::upper)
  int64_t mrows = 0, lda = 0;  // (OP_KERNEL_PRECOND: mrows is the factor's padded rank)
  int has_tiles = 0;        // workgroup tiles (tiles.tile_ptr)
  int tiles_ringed = 0;     // ... built to the caps of the ring-fed kernels
  int tiles_max_cols = 0;   // longest line list of a tile
  double upper_per_row = 0.0;  // distinct panel rows per row the upper-triangle stream lands
  int upper_stream = 0;     // an upper-triangle tile stream exists (streams[0].upper)
  int upper_padded = 0;     // ... with its rows padded to whole chunks
  double far_per_row = 0.0;
  int affine = 0;           // A + t B: vals_b is set
  int32_t xcd_tile[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};    // tile ranges per XCD chunk: the base tiles,
  int32_t xcd_tile_u[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // the upper-triangle stream,
  struct Merged {           // and the merged streams of narrow panels, [0] R = 2, [1] R = 4 (one partition for both triangles)
    int available = 0;      // built (slq.hip builds it when wants_merged_stream says so, before it takes these facts)
    int upper = 0, u_padded = 0;
    int32_t xcd_tile[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  } merged[2];
  // context
  int num_cus = 0;
  // request (deg and orth as normalise_params leaves them)
  int nprobes = 0, deg = 0, orth = 0;
  PlanKind plan = PlanKind::Ring;
};
constexpr int kNumPlanFacts = 16 + 18 + 2 * 12 + 5;

inline PlanFacts plan_facts_from_array(const double *a) {
  PlanFacts f;
  int i = 0;
  f.kind = (int)a[i++], f.dtype = (int)a[i++];
  f.n = (int64_t)a[i++], f.nnz = (int64_t)a[i++], f.nnz_u = (int64_t)a[i++];
  f.upper = (int)a[i++];
  f.mrows = (int64_t)a[i++], f.lda = (int64_t)a[i++];
  f.has_tiles = (int)a[i++], f.tiles_ringed = (int)a[i++], f.tiles_max_cols = (int)a[i++];
  f.upper_per_row = a[i++];
  f.upper_stream = (int)a[i++], f.upper_padded = (int)a[i++];
  f.far_per_row = a[i++];
  f.affine = (int)a[i++];
  for (int x = 0; x < 9; ++x) f.xcd_tile[x] = (int32_t)a[i++];
  for (int x = 0; x < 9; ++x) f.xcd_tile_u[x] = (int32_t)a[i++];
  for (PlanFacts::Merged &m : f.merged) {
    m.available = (int)a[i++], m.upper = (int)a[i++], m.u_padded = (int)a[i++];
    for (int x = 0; x < 9; ++x) m.xcd_tile[x] = (int32_t)a[i++];
  }
  f.num_cus = (int)a[i++];
  f.nprobes = (int)a[i++], f.deg = (int)a[i++], f.orth = (int)a[i++];
  f.plan = (PlanKind)(int)a[i++];
  return f;
}
inline void plan_facts_to_array(const PlanFacts &f, double *a) {
  int i = 0;
  a[i++] = f.kind, a[i++] = f.dtype;
  a[i++] = (double)f.n, a[i++] = (double)f.nnz, a[i++] = (double)f.nnz_u;
  a[i++] = f.upper;
  a[i++] = (double)f.mrows, a[i++] = (double)f.lda;
  a[i++] = f.has_tiles, a[i++] = f.tiles_ringed, a[i++] = f.tiles_max_cols;
  a[i++] = f.upper_per_row;
  a[i++] = f.upper_stream, a[i++] = f.upper_padded;
  a[i++] = f.far_per_row;
  a[i++] = f.affine;
  for (int x = 0; x < 9; ++x) a[i++] = f.xcd_tile[x];
  for (int x = 0; x < 9; ++x) a[i++] = f.xcd_tile_u[x];
  for (const PlanFacts::Merged &m : f.merged) {
    a[i++] = m.available, a[i++] = m.upper, a[i++] = m.u_padded;
    for (int x = 0; x < 9; ++x) a[i++] = m.xcd_tile[x];
  }
  a[i++] = f.num_cus;
  a[i++] = f.nprobes, a[i++] = f.deg, a[i++] = f.orth;
  a[i++] = (int)f.plan;
}

// ---- the workspace table ---------------------------------------------------------------------------------------------
// One region per device allocation a creation makes, in allocation order. bytes == 0: not allocated for this plan.
// zeroed: 0 left as allocated, 1 cleared (synchronously) when allocated, 2 cleared on the plan's stream once everything is
// allocated. counted: the region enters slq_plan_workspace_bytes - the panels and the arrays that grow with deg * probes. Left
// out, as they always were: the four counters of sweep_cols, the state of the edge recurrence (om_*: 4 doubles per probe, two
// flags per step and panel), the active block (two ints per probe), the outside flags and the coefficients of a Chebyshev plan.
enum WorkspaceId {
  WS_RING = 0,    // S slots of NP panels (+ stash and output panel of a recompute plan, + the output panel of an action plan)
  WS_SCAL,        // one allocation behind the StepState arrays (ScalOffsets)
  WS_PART,        // [kReorthChunk][part_maxblk][bpad] partial sums
  WS_ACC_COEF,    // recompute: [deg][bpad] coefficients of the action
  WS_SWEEP_COLS,  // 4 counters (slq_plan_sweep_columns, slq_plan_action_columns)
  WS_OM_BUF, WS_OM_FLAGS, WS_OM_CNT,  // the edge recurrence (omega_on)
  WS_OM_CENSUS,   // SLQ_OMEGA=2 on a ring-fed Gram plan
  WS_ACTIVE,      // active[bpad] | steps[bpad] | fail_d, ring_fail_d, fail_d[2] (ActiveOffsets)
  WS_QUAD,        // quad[bpad] | nodes[hist][bpad] | weights[hist][bpad]
  WS_CHEB_MU, WS_CHEB_OUT, WS_CHEB_COEF,
  WS_T,           // product panel of dense / callback / Gram operators, the K-split slabs of the big-tile dense kernels behind it
  WS_T2,          // Gram: the m-row intermediate; preconditioned kernel operator: V and scratch; Toeplitz: the complex workspace of the multi-kernel product
  kNumRegions
};
struct Region {
  int id = 0;
  size_t bytes = 0;
  int zeroed = 0, counted = 0;
};
// where the StepState arrays begin inside WS_SCAL, in doubles; `end` is the region's size
struct ScalOffsets {
  size_t alpha = 0, nu_margin = 0, nu = 0, vnorm2 = 0, coefA = 0, coefB = 0, cross = 0, gram = 0, gamma = 0, end = 0;
};
// ... and the sub-arrays of WS_ACTIVE, in ints (active itself is at 0)
struct ActiveOffsets {
  size_t steps = 0, fail = 0, ring_fail = 0, fail2 = 0, end = 0;
};

// Which kernel computes a plan's dense product (the ids of slq_plan_dense_path). 0: not a dense operator.
enum { DENSE_K_NONE = 0, DENSE_K_PANEL = 1, DENSE_K_3TERM = 2, DENSE_K_TILE = 3, DENSE_K_LDS = 4, DENSE_K_LDS32 = 5 };
// the tile stream a plan's ring-fed passes read
enum { STREAM_NONE = 0, STREAM_BASE = 1, STREAM_MERGED2 = 2, STREAM_MERGED4 = 3 };

// The whole decision.
struct PlanShape {
  int LPR = 0, PW = 0, NP = 0, bpad = 0;
  int S = 0;                  // ring slots
  int acc_cols = 0;           // finished ring columns one accumulation launch consumes (recompute, action plans)
  int v_slot = 0, y_slot = 0; // where an action's probes and its output are
  int64_t slot_stride = 0;    // elements between ring slots
  int rmax = 0;
  int hist = 0;               // rows of alpha / nu beyond row 0, columns of the stored Gauss rule
  int pipelined = 0;
  int nblkA = 0, nblkS = 0, nblkU = 0, nblkF = 0, nblkT = 0;  // grids: SpMM, streaming sweeps, fused dots/update, fused alpha, tiled passes
  size_t alpha_pad = 0;       // LDS padding that caps the alpha pass's residency
  int part_maxblk = 0;
  int dense_ks = 0;           // K split of the big-tile dense kernels (0: none of them)
  // T as the one-shot entries estimate it BEFORE a plan exists (plan_estimate_bytes): 1 + 16 slabs wherever the panel width
  // admits a big-tile kernel, whatever the switches and the dense_ks search will say. A bound (dense_ks <= 16), deliberately
  // not the exact 1 + dense_ks: the entries chunk their probes by it, and a tighter estimate would change the chunks - and
  // with them the bits of their results.
  int t_slabs_bound = 0;
  int dense_class = 0;        // DENSE_K_*
  int ringR = 0;              // panel rows per wave instruction of the tile stream the plan uses (0: no tiles)
  int stream = STREAM_NONE;
  int rs_upper = 0;           // ... with an upper-triangle stream for the alpha-only pass
  int rs_u_padded = 0, ring_staged = 0;
  int32_t rs_xcd[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, rs_xcd_u[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  int omega_on = 0;
  seq::SequenceFacts seq;     // the facts of step_shape with their derived flags, at nstale = 0
  Region ws[kNumRegions];
  ScalOffsets scal;
  ActiveOffsets active;
};
constexpr int kNumPlanShape = 27 + 18 + 6 + 4 * kNumRegions + 10 + 5;

inline void plan_shape_to_array(const PlanShape &s, double *a) {
  int i = 0;
  a[i++] = s.LPR, a[i++] = s.PW, a[i++] = s.NP, a[i++] = s.bpad, a[i++] = s.S, a[i++] = s.acc_cols, a[i++] = s.v_slot, a[i++] = s.y_slot;
  a[i++] = (double)s.slot_stride, a[i++] = s.rmax, a[i++] = s.hist;
  a[i++] = s.pipelined, a[i++] = s.nblkA, a[i++] = s.nblkS, a[i++] = s.nblkU, a[i++] = s.nblkF, a[i++] = s.nblkT;
  a[i++] = (double)s.alpha_pad, a[i++] = s.part_maxblk, a[i++] = s.dense_ks, a[i++] = s.t_slabs_bound, a[i++] = s.dense_class;
  a[i++] = s.ringR, a[i++] = s.stream, a[i++] = s.rs_upper, a[i++] = s.rs_u_padded, a[i++] = s.ring_staged;
  for (int x = 0; x < 9; ++x) a[i++] = s.rs_xcd[x];
  for (int x = 0; x < 9; ++x) a[i++] = s.rs_xcd_u[x];
  a[i++] = s.omega_on, a[i++] = s.seq.ring_gen, a[i++] = s.seq.ring_deep, a[i++] = s.seq.gram, a[i++] = s.seq.gram_csr, a[i++] = s.seq.last_nostore;
  for (const Region &r : s.ws) a[i++] = r.id, a[i++] = (double)r.bytes, a[i++] = r.zeroed, a[i++] = r.counted;
  const ScalOffsets &o = s.scal;
  for (size_t v : {o.alpha, o.nu_margin, o.nu, o.vnorm2, o.coefA, o.coefB, o.cross, o.gram, o.gamma, o.end}) a[i++] = (double)v;
  for (size_t v : {s.active.steps, s.active.fail, s.active.ring_fail, s.active.fail2, s.active.end}) a[i++] = (double)v;
}

// ---- geometry ----------------------------------------------------------------------------------------------------------
inline size_t esize_of(int dtype) { return dtype == kF64 ? 8 : 4; }

inline void choose_geometry(const PlanSwitches &sw, int dtype, int nprobes, int *LPR, int *PW, int *NP) {
  const int V = dtype == kF64 ? 2 : 4;
  int lpr = 8;
  while (lpr < 64 && lpr * V < nprobes) lpr *= 2;
  const int forced = sw.lpr;
  if (forced == 8 || forced == 16 || forced == 32 || forced == 64) lpr = forced;
  *LPR = lpr;
  *PW = lpr * V;
  *NP = (nprobes + *PW - 1) / *PW;
}

inline int ring_slots(int deg, int orth, int keep_basis) {
  if (keep_basis) return deg + 1;
  if (orth == 0) return 2;
  return std::max(orth + 1, 3);
}

// A recompute plan's ring: the quadrature plan's, widened until an accumulation launch finds acc finished columns beside the one
// the step wrote (acc + 1 slots), acc = min(kAccCols, deg). At most kAccCols slots more, none when orth >= kAccCols.
inline int recompute_acc_cols(int deg) { return std::min(kAccCols, deg); }
inline int recompute_ring_slots(int deg, int orth) { return std::max(ring_slots(deg, orth, 0), recompute_acc_cols(deg) + 1); }

inline void grid_sizes(const PlanSwitches &sw, int64_t n, int LPR, int NP, int num_cus, int *nblkA, int *nblkS, int *nblkU, bool pipelined) {
  const int RPW = 64 / LPR;
  const int rows_per_block = kWaves * RPW;
  // Tunables: resident workgroups (kBlock threads) per CU, summed over the panels of a launch.
  // Defaults from the MI355X sweeps: in-place read-modify-write sweeps peak at
  // ~2 workgroups per CU (more concurrent writers lose 5-10 %); the SpMM likes 4-8.
  const int per_cu_a = std::max(1, or_auto(sw.blocks_per_cu_spmm, or_auto(sw.blocks_per_cu, 4)));
  const int per_cu_s = std::max(1, or_auto(sw.blocks_per_cu_stream, or_auto(sw.blocks_per_cu, 2)));
  // sweep A: a multiple of 8 blocks (XCD-aware chunking), no more than the rows can feed
  const int64_t chunk = (n + 7) / 8;
  const int64_t chunk_blocks = (chunk + rows_per_block - 1) / rows_per_block;
  int per_xcd = (int)std::min<int64_t>(std::max(8, num_cus * per_cu_a / NP) / 8, chunk_blocks);
  per_xcd = std::max(per_xcd, 1);
  *nblkA = 8 * per_xcd;
  // fused dots/update passes: 2 workgroups resident per CU (LDS padding, enqueue_run) and a grid of 2 per CU
  // per panel. More rows in flight evict each other's gather halo
  // (dots pass, r = 3, per 30 launches: 36.3 ms at 2 resident, 41.3 at 3), and a grid that is not a multiple
  // of what is resident leaves a ragged last round. Panels run one after the other (panel-major dispatch).
  const int per_cu_u = std::max(1, or_auto(sw.blocks_per_cu_fused, pipelined ? 1 : 2));  // per panel; 1 with the pipelined row loop
  const int per_xcd_u = (int)std::min<int64_t>(std::max(8, num_cus * per_cu_u) / 8, chunk_blocks);
  *nblkU = 8 * std::max(per_xcd_u, 1);
  const int s = (int)std::min<int64_t>(std::max(1, num_cus * per_cu_s / NP), (n + rows_per_block - 1) / rows_per_block);
  *nblkS = std::max(s, 1);
}

// The merged tiles of narrow panels are built on first use, which is device work: slq.hip builds the stream of R = the answer
// (2 or 4; 0: none wanted) BEFORE it takes the facts, and records the outcome in PlanFacts::merged.
inline int wants_merged_stream(const PlanFacts &f, const PlanSwitches &sw) {
  int LPR, PW, NP;
  choose_geometry(sw, f.dtype, f.nprobes, &LPR, &PW, &NP);
  const bool wanted = (LPR == 32 || LPR == 16) && f.tiles_ringed && sw.nt && sw.ring_narrow != 0 && f.kind == OP_CSR && f.has_tiles && sw.tiles;
  return wanted ? 64 / LPR : 0;
}

inline PlanShape plan_shape(const PlanFacts &f, const PlanSwitches &sw) {
  PlanShape s;
  const bool cheb = is_cheb(f.plan), action = f.plan == PlanKind::ChebyshevAction, recompute = f.plan == PlanKind::Recompute;
  const bool keep_basis = f.plan == PlanKind::KeepBasis;
  const int deg = f.deg, orth = f.orth;
  const size_t esz = esize_of(f.dtype);
  s.hist = cheb ? 0 : deg;
  choose_geometry(sw, f.dtype, f.nprobes, &s.LPR, &s.PW, &s.NP);
  s.bpad = s.NP * s.PW;
  s.S = recompute ? recompute_ring_slots(deg, orth) : ring_slots(deg, orth, keep_basis);
  s.acc_cols = recompute ? recompute_acc_cols(deg) : 0;
  s.v_slot = recompute ? s.S : 0;
  s.y_slot = recompute ? s.S + 1 : deg;
  if (action) {
    s.S = seq::cheb_action_ring_slots(deg, kChebAccCols);
    s.acc_cols = kChebAccCols;
    s.y_slot = s.S;  // (the output panel behind the ring; the probes are ring column 0: no stash)
  }
  s.slot_stride = (int64_t)s.NP * f.n * s.PW;
  s.rmax = std::max(keep_basis ? deg : orth, 1);
  // Row loop of the dots/update passes (slq_kernels.hpp: k_csr_pass). Measured on configs[1] and on the 100^3 grid
  // (DESIGN.md §5.3): rows of up to 5 nonzeros are fastest with the plain loop at 2 resident workgroups per CU (82.9
  // against 91.7 ms per step), 7-point rows with the pipelined loop at ONE resident workgroup per CU (93.7 against
  // 101.0 ms): what bounds both is the traffic a CU's vector-memory pipe has in flight, and the pipelined loop puts
  // the same bytes in flight with half the waves.
  s.pipelined = f.kind == OP_CSR && s.LPR == 64 && (sw.pipe >= 0 ? sw.pipe != 0 : (double)f.nnz / (double)std::max<int64_t>(f.n, 1) > 5.5);
  grid_sizes(sw, f.n, s.LPR, s.NP, f.num_cus, &s.nblkA, &s.nblkS, &s.nblkU, s.pipelined != 0);
  {
    // Fused alpha pass: one read sweep plus the gathers. Two regimes, told apart by the
    // gathers per row of the matrix the pass walks (upper triangle when the operator is symmetric):
    //  * <= 3 (5-point stencil, upper triangle): each wave has too few loads in flight, the pass is bound by
    //    the rowptr -> colind -> gather latency chain: 4 workgroups per CU in total, panels side by side
    //    (configs[1]: 0.88 ms at 2 per CU, 0.51 at 4; one panel at a time with 4 resident 0.61);
    //  * more (full 5-point rows: 0.92 ms at 2 per CU vs 0.96 at 4; 7-point upper triangle: 0.67 vs 0.83;
    //    random graphs): the waves carry enough loads and extra rows in flight only evict each other's halo
    //    from the XCD's L2: 2 resident per CU (LDS padding), 2 per CU *per panel*, panel after panel.
    const double gathers = f.kind != OP_CSR ? 0.0 : (double)(f.upper ? f.nnz_u : f.nnz) / (double)std::max<int64_t>(f.n, 1);
    const int local = f.kind == OP_CSR && gathers <= 3.2;
    const int per_cu_env = sw.blocks_per_cu_alpha;  // total over the panels
    const int rows_per_block = kWaves * (64 / s.LPR);
    const int64_t chunk = (f.n + 7) / 8;
    const int per_panel = per_cu_env > 0 ? std::max(8, f.num_cus * per_cu_env / s.NP)
                                         : (local ? std::max(8, f.num_cus * 4 / s.NP) : f.num_cus * 2);
    const int per_xcd = (int)std::min<int64_t>(per_panel / 8, (chunk + rows_per_block - 1) / rows_per_block);
    s.nblkF = 8 * std::max(per_xcd, 1);
    s.alpha_pad = (size_t)or_auto(sw.alpha_lds_pad, (per_cu_env > 0 || local) ? 0 : 65536);
  }
  {
    // which tile stream, if any (plan_tiled): wide panels take the tiles as clustered; panels of 32 / 16 lanes per row the
    // merged tiles of the narrow-panel ring kernel (built on first use; nontemporal streams only - the one form instantiated)
    for (int x = 0; x < 9; ++x) s.rs_xcd[x] = f.xcd_tile[x], s.rs_xcd_u[x] = f.xcd_tile_u[x];
    if (f.kind == OP_CSR && f.has_tiles && sw.tiles) {
      const int R = wants_merged_stream(f, sw);
      if (s.LPR == 64) {
        s.ringR = 1;
        if (f.tiles_ringed) {
          s.stream = STREAM_BASE;
          if (f.upper_stream && f.upper_per_row <= (double)sw.ring_alpha_max_x100 / 100.0)  // (default: kTileAlphaColsPerRow)
            s.rs_upper = 1, s.rs_u_padded = f.upper_padded;
        }
      } else if (R && f.merged[R == 2 ? 0 : 1].available) {
        const PlanFacts::Merged &m = f.merged[R == 2 ? 0 : 1];
        s.ringR = R;
        s.stream = R == 2 ? STREAM_MERGED2 : STREAM_MERGED4;
        s.rs_upper = m.upper, s.rs_u_padded = m.u_padded;
        for (int x = 0; x < 9; ++x) s.rs_xcd[x] = m.xcd_tile[x], s.rs_xcd_u[x] = m.xcd_tile[x];  // (merged streams: one partition for both)
      }
      // alpha-only pass: LDS-DMA loaders everywhere since their r03 rewrite (merged tiles: a lane reads its lines' sources straight
      // out of the staged descriptor - 100^3, 64 probes 0.230 -> 0.187 ms against the register-staged loaders that had been the
      // faster form there, configs[1] 0.129 -> 0.113). SLQ_RING_STAGED=1 takes the loaders through registers (GEO 1) again.
      s.ring_staged = sw.ring_staged != 0;
    }
  }
  {
    // tiled passes: as many workgroups resident per CU as their LDS images admit (2 x 72 KiB by default), the same number
    // per CU and panel in the grid, panel after panel
    const int img_kib = f.has_tiles ? (f.tiles_max_cols + 16) * (SLQ_TILE_DB ? 2 : 1) : 160;
    const int per_cu_t = f.tiles_ringed ? 1 : std::max(1, or_auto(sw.blocks_per_cu_tiled, std::max(1, std::min(4, 160 / std::max(img_kib, 1)))));
    int per_xcd_t = std::max(1, f.num_cus * per_cu_t / 8);
    per_xcd_t = std::max(1, std::min(per_xcd_t, or_auto(sw.tiled_wgs_per_xcd, per_xcd_t)));  // (experiments: fewer CUs sweeping a chunk)
    if (f.has_tiles) {
      int mn = 1 << 30;
      for (int x = 0; x < 8; ++x) mn = std::min(mn, std::max(1, s.rs_xcd[x + 1] - s.rs_xcd[x]));
      per_xcd_t = std::min(per_xcd_t, mn);
    }
    s.nblkT = 8 * per_xcd_t;
  }
  s.part_maxblk = std::max(std::max(std::max(std::max(s.nblkA, s.nblkF), s.nblkU), s.nblkS), s.nblkT);
  // dense fp64 operator on the matrix cores with 32-row tiles: n/32 workgroups per panel rarely fill 256 CUs, so K is
  // also split over dense_ks workgroups whose raw products land in dense_ks slabs behind T. ks minimises the number
  // of workgroup rounds times the work per workgroup, plus a small cost per slab.
  s.dense_ks = 0;  // 0: the 16-row kernel with its fused epilogue
  const bool dense32 = f.kind == OP_DENSE && f.dtype == kF32 && sw.dense_mfma;  // fp32: k_dense_mfma32_lds, 256-row tiles, every panel width
  if (dense32 || (f.kind == OP_DENSE && f.dtype == kF64 && sw.dense_mfma && s.PW >= 32 && !sw.dense_tile16)) {
    const int rw = dense32 ? kDense32BM : 32 * (kWaves / (s.PW >= 64 ? 2 : 1));
    const double wgs = (double)((f.n + rw - 1) / rw) * s.NP;
    double best = 1e30;
    const int forced = sw.dense_ksplit;
    for (int ks = 1; ks <= 16; ++ks) {
      const double cost = std::ceil(wgs * ks / f.num_cus) / ks + 0.005 * ks;
      if ((forced > 0 && ks == forced) || (forced <= 0 && cost < best - 1e-12)) { best = cost; s.dense_ks = ks; }
    }
  }
  // kernel operator (slq_kernelop.hpp): the j slabs of its product take the same place behind T (dense_ks slabs; 0: one slab, straight into T)
  if (is_kernel_kind(f.kind)) {
    const int slabs = kernel_schedule(f.n, s.PW, s.NP, f.num_cus).nslabs;
    s.dense_ks = slabs > 1 ? slabs : 0;
  }
  s.t_slabs_bound = f.kind == OP_CSR ? 0 : 1 + (((f.kind == OP_DENSE && (f.dtype == kF32 || s.PW >= 32)) || is_kernel_kind(f.kind)) ? 16 : 0);
  // the one decision behind launch_dense_mfma, apply_operator_unfused and the step loop
  if (f.kind != OP_DENSE) s.dense_class = DENSE_K_NONE;
  else if (!sw.dense_mfma || (f.dtype != kF64 && s.dense_ks <= 0)) s.dense_class = DENSE_K_PANEL;  // the VALU kernel (SLQ_DENSE_MFMA=0)
  else if (s.dense_ks <= 0) s.dense_class = DENSE_K_3TERM;  // 16-column panels, SLQ_DENSE_TILE16=1: the 16-row kernel with its fused epilogue
  else if (f.dtype == kF32) s.dense_class = DENSE_K_LDS32;
  // operands staged in LDS once per workgroup: 16-byte aligned row pairs (lda even) and panels of 64+ columns (32-column
  // panels keep the register form: their 256-row block does not fit static LDS)
  else s.dense_class = sw.dense_lds && f.lda % 2 == 0 && s.PW >= 64 ? DENSE_K_LDS : DENSE_K_TILE;
  // which form of the ring-fed passes, and which steps take the Gram sequence (derive_plan_flags, slq_sequence.hpp). The Gram sequence
  // needs an EXACTLY symmetric operator: it rewrites W_t . (A W_j) as (A W_t) . W_j - §4.6 - while the reference's recurrence never looks
  // at symmetry, lanczos.h:127-136; `upper` is the record of that check (r04: r03 took the sequence on any tiled operator).
  // The Gram sequence on the generic passes (no tiles, or a plan whose panels the tiles do not serve): the dots pass - a third to a half of every
  // step's bytes - is gone there as well. Not for operators whose gathers are the cost (random graphs keep the stored-u sequence: it gathers once,
  // the Gram sequence twice) - step_shape decides that per step.
  {
    seq::SequenceFacts &q = s.seq;
    q.csr = f.kind == OP_CSR, q.far_le4 = f.far_per_row <= 4.0, q.tiles_ringed = f.tiles_ringed, q.upper = f.upper;
    q.ringR = s.ringR, q.rs_desc_u = s.rs_upper, q.rs_u_padded = s.rs_u_padded;
    q.deg = deg, q.orth = orth, q.nstale = 0, q.basis_mode = basis_mode_of(f.plan);
    q.dense_class = s.dense_class, q.pipelined = s.pipelined;
    q.fused = sw.fused, q.merged = sw.merged, q.mgs = sw.mgs, q.stored_u = sw.stored_u, q.nt = sw.nt, q.cross = sw.cross, q.sw_gram = sw.gram;
    q.sw_gram_csr = sw.gram_csr, q.sw_ring_gen = sw.ring_gen, q.sw_ring_deep = sw.ring_deep;
    q.last_store = (sw.last_store == 1 || action) ? 1 : 0;  // (an action reads w_nsteps: the last step stores it)
    q.ring_alpha = sw.ring_alpha, q.ring_rev = sw.ring_rev;
    seq::derive_plan_flags(q);  // (the derived flags do not depend on omega_on)
    // the edge recurrence: full windows of three columns on the ring-fed Gram sequence (r = 4 .. 8: not offered; the rescue needs the
    // column that leaves the window still in the ring: orth + 1 slots at least)
    // (panels of 32 columns at least: the bound of the rescue's former second kernel, whose early exit looked at the first and the last
    // panel under a block of 64 columns; the single launch does not need it, the plans that are offered stay the same)
    s.omega_on = q.gram && sw.omega != 0 && orth == 3 && s.S >= 4 && !f.affine && s.PW >= 32;
    q.omega_on = s.omega_on;
  }

  // ---- the workspace table ----
  const size_t bp = (size_t)s.bpad, hist = (size_t)s.hist;
  const size_t slot_bytes = (size_t)s.slot_stride * esz;
  for (int r = 0; r < kNumRegions; ++r) s.ws[r].id = r;
  auto region = [&s](int id, size_t bytes, int zeroed, int counted) { s.ws[id].bytes = bytes, s.ws[id].zeroed = zeroed, s.ws[id].counted = counted; };
  // (recompute: stash and output behind the ring; Chebyshev action: the output)
  region(WS_RING, (size_t)(s.S + (recompute ? 2 : (action ? 1 : 0))) * slot_bytes, 0, 1);
  {
    // alpha[hist+1], nu[orth margin for stale vectors t < 0 | hist+1], vnorm2, coefA[2], coefB, cross, gram[2][kFusedMaxR+1], gamma[rmax]
    ScalOffsets &o = s.scal;
    size_t at = 0;
    o.alpha = at, at += (hist + 1) * bp;
    o.nu_margin = at, at += (size_t)orth * bp;  // nu rows for t = -orth .. -1 (zero unless the drop-in entry preloads stale columns)
    o.nu = at, at += (hist + 1) * bp;
    o.vnorm2 = at, at += bp;
    o.coefA = at, at += 2 * bp;
    o.coefB = at, at += bp;
    o.cross = at, at += bp;
    o.gram = at, at += (size_t)2 * (kFusedMaxR + 1) * bp;
    o.gamma = at, at += (size_t)s.rmax * bp;
    o.end = at;
    region(WS_SCAL, o.end * 8, 2, 1);
  }
  region(WS_PART, (size_t)kReorthChunk * s.part_maxblk * bp * 8, 0, 1);
  region(WS_ACC_COEF, recompute ? (size_t)deg * bp * 8 : 0, 0, 1);
  region(WS_SWEEP_COLS, 4 * sizeof(unsigned long long), 1, 0);  // (words 2, 3: the accumulation launches of a recompute plan, slq_plan_action_columns)
  region(WS_OM_BUF, s.omega_on ? 4 * bp * 8 : 0, 1, 0);
  region(WS_OM_FLAGS, s.omega_on ? (size_t)2 * (deg + 1) * s.NP * sizeof(int) : 0, 1, 0);
  region(WS_OM_CNT, s.omega_on ? 8 * sizeof(unsigned long long) : 0, 1, 0);
  region(WS_OM_CENSUS, (s.seq.gram && sw.omega == 2 && !cheb) ? (size_t)(deg + 1) * (kFusedMaxR + 1) * s.NP * sizeof(int) : 0, 1, 0);
  {
    ActiveOffsets &o = s.active;
    o.steps = bp, o.fail = 2 * bp, o.ring_fail = o.fail + 1, o.fail2 = o.fail + 2, o.end = o.fail + 4;
    region(WS_ACTIVE, o.end * sizeof(int), 0, 0);
  }
  region(WS_QUAD, (bp + 2 * bp * hist) * 8, 0, 1);
  const size_t nmom = cheb ? (size_t)(2 * deg + 1) : 0;  // moments per probe (256 probes, 16384 steps: 67 MB)
  region(WS_CHEB_MU, nmom * bp * 8, 1, 1);
  region(WS_CHEB_OUT, cheb ? bp * sizeof(int) : 0, 1, 0);
  region(WS_CHEB_COEF, cheb ? (nmom + 4) * 8 : 0, 0, 0);
  region(WS_T, f.kind == OP_CSR ? 0 : (size_t)(1 + s.dense_ks) * slot_bytes, 0, 1);
  // (preconditioned kernel operator: V = M W_c, then the slab partials and G L^T W of an apply - scratch of the PLAN, whose captured graphs hold its addresses)
  region(WS_T2, f.kind == OP_GRAM             ? (size_t)s.NP * (size_t)f.mrows * s.PW * esz
                : f.kind == OP_KERNEL_PRECOND ? slot_bytes + precond_scratch_words(f.n, s.bpad, (int)f.mrows, f.num_cus) * 8
                // (Toeplitz operator, DESIGN.md §4.24: L x PW words, ONE panel in flight - the panels of a product run one after the other)
                : f.kind == OP_TOEPLITZ       ? toeplitz_plan(f.n, (int)esz, s.PW).ws_bytes
                                              : 0, 0, 1);
  return s;
}

// slq_plan_workspace_bytes: the counted regions
inline size_t plan_workspace_bytes(const PlanShape &s) {
  size_t b = 0;
  for (const Region &r : s.ws)
    if (r.counted) b += r.bytes;
  return b;
}

// What a plan on an operator allocates, as the one-shot entries ask BEFORE they create it: the ring plus the product panels of
// operators that are not applied row by row inside the passes - T at its bound of t_slabs_bound slabs (see there) and T2. The
// scalar arrays (and a recompute plan's coefficient buffer: 1 MB at deg 512, 256 probes) are left out: the callers keep 1 GiB
// of margin.
inline size_t plan_estimate_bytes(const PlanShape &s, const PlanFacts &f) {
  return s.ws[WS_RING].bytes + (size_t)s.t_slabs_bound * (size_t)s.slot_stride * esize_of(f.dtype) + s.ws[WS_T2].bytes;
}

}  // namespace slq
