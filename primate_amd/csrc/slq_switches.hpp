// slq_switches.hpp — every run-time switch of the library: ONE table, one line per switch, read from the
// environment at one of two moments and never again.
//   OP   when an operator is created (OperatorSwitches, stored on the operator: everything built for it later - the merged
//        streams of narrow panels included - is built under the values it was created with)
//   PLAN when a plan is created (PlanSwitches, stored on the plan: a plan never changes its behaviour afterwards; the byte
//        queries that size a plan before it exists read the same table)
//   BOTH at both moments (each object keeps the value of its own moment)
//   USE  where it is used (SLQ_HOST_THREADS only: a thread count, which no result depends on)
// Plain C++. The table is the only place a switch's name appears as a string, and env_int the only caller of getenv.
#pragma once

#include <climits>
#include <cstdlib>

namespace slq {

constexpr int kAuto = INT_MIN;  // "unset": the code that uses the switch picks the value (the table's meaning column says how)

//        field, name, default, meaning
#define SLQ_SWITCH_TABLE(OP, PLAN, BOTH, USE)                                                                                                            \
  BOTH(tiles, "SLQ_TILES", 2, "LDS workgroup tiles: 0 none, 1 landed behind barriers, 2 fed through a ring of LDS slots; operator: rows regrouped, plan: passes use them") \
  OP(debug, "SLQ_DEBUG", 0, "print the phases and findings of an operator's creation on stderr")                                                      \
  OP(reorder, "SLQ_REORDER", -1, "XCD-aware RCM row order: 0 never, 1 n >= 65536, 2 always, -1 automatic")                                            \
  OP(rcm_sub, "SLQ_RCM_SUB", 0, "second reordering level: runs of Cuthill-McKee levels per XCD chunk (0: 1, and what the tile sweep finds)")           \
  OP(sym_alpha, "SLQ_SYM_ALPHA", 1, "alpha pass on the upper triangle of an exactly symmetric CSR")                                                  \
  OP(tile_rows, "SLQ_TILE_ROWS", 24, "tile caps of the barrier tiles: rows")                                                                         \
  OP(tile_cols, "SLQ_TILE_COLS", 72, "... distinct panel rows")                                                                                      \
  OP(device_build, "SLQ_DEVICE_BUILD", 1, "operators with ring tiles built on the device (0: on the host; 2: both, compared byte for byte)")          \
  OP(ring_order, "SLQ_RING_ORDER", 0, "order of a tile's lines (1: own rows first; experiments)")                                                    \
  OP(ring_upper_regroup, "SLQ_RING_UPPER_REGROUP", 1, "upper-triangle tiles regrouped into runs of the base tiles")                                  \
  OP(ring_pad_rows, "SLQ_RING_PAD_ROWS", 1, "upper-triangle tile streams with every row padded to whole chunks of four entries")                     \
  USE(host_threads, "SLQ_HOST_THREADS", kAuto, "host threads of operator creation and of the pinned probe upload (auto: min(16, hardware threads))")  \
  PLAN(fused, "SLQ_FUSED", 1, "1: recompute-SpMM passes where they pay, 0: store-and-revisit sweeps, 2: passes always")                               \
  PLAN(nt, "SLQ_NT", 1, "nontemporal hints on streamed-once rows")                                                                                   \
  PLAN(graph, "SLQ_GRAPH", 1, "capture the launch sequence into a hipGraph")                                                                         \
  PLAN(mgs, "SLQ_MGS", 0, "exact modified-Gram-Schmidt order")                                                                                       \
  PLAN(stored_u, "SLQ_STORED_U", 1, "non-local operators: merged pass stores u, update pass reads it back")                                          \
  PLAN(merged, "SLQ_MERGED", 1, "alpha from the merged alpha+dots pass")                                                                             \
  PLAN(cross, "SLQ_CROSS", 1, "q_c.q_p from the update pass's cross term")                                                                           \
  PLAN(gram, "SLQ_GRAM", 1, "Gram sequence: projections from Gram rows of the update passes")                                                        \
  PLAN(gram_csr, "SLQ_GRAM_CSR", 1, "... also on the generic passes (plans without ring-fed tiles)")                                                 \
  PLAN(ring_gen, "SLQ_RING_GEN", 1, "wide-panel ring-fed passes through k_ring_pass (0: k_csr_ring_pass)")                                           \
  PLAN(ring_deep, "SLQ_RING_DEEP", 1, "steps with 4..8 ring columns on the 8-wave form of k_ring_pass (0: generic passes)")                          \
  PLAN(ring_narrow, "SLQ_RING_NARROW", 1, "panels of 32 / 16 lanes per row on merged tiles (0: generic passes on the tiles' row order)")             \
  PLAN(ring_staged, "SLQ_RING_STAGED", 0, "alpha-only pass: loader waves through registers instead of LDS-DMA")                                      \
  PLAN(ring_alpha, "SLQ_RING_ALPHA", 2, "alpha-only pass of a tiled symmetric operator: 2 ring over the upper-triangle stream, 1 over full rows, 0 generic") \
  PLAN(ring_alpha_max_x100, "SLQ_RING_ALPHA_MAX_X100", 260, "... takes the upper-triangle stream up to this many (x100) landed rows per row")        \
  PLAN(ring_rev, "SLQ_RING_REV", 1, "the ring-fed update pass sweeps panels and tiles in reverse")                                                   \
  PLAN(last_store, "SLQ_LAST_STORE", 0, "the update pass of a run's last step: 0 stores nothing and is launched when beta_deg is first asked for, 1 stores W_deg although it is never read, 2 stores nothing, launched with the run") \
  PLAN(sweep_skip, "SLQ_SWEEP_SKIP", 1, "the update sweep skips ring columns whose coefficient is zero for the whole panel")                         \
  PLAN(acc_skip, "SLQ_ACC_SKIP", 1, "the accumulation of a recompute plan's replay skips such columns")                                              \
  PLAN(defer_axpy, "SLQ_DEFER_AXPY", 1, "block-CGS sweeps: the dots sweeps are read-only, the update sweep applies the three-term axpy")             \
  PLAN(omega, "SLQ_OMEGA", 1, "edge recurrence: 1 on, 0 every column read, 2 verify (clamped to 0..2)")                                              \
  PLAN(omega_trip, "SLQ_OMEGA_TRIP", -1, "tests: the step at which every panel reads (-1: none)")                                                    \
  PLAN(omega_rescue, "SLQ_OMEGA_RESCUE", -1, "tests: the step at which every panel takes the rescue (-1: none)")                                     \
  PLAN(dense_mfma, "SLQ_DENSE_MFMA", 1, "dense operator on the matrix cores (0: k_dense_panel)")                                                     \
  PLAN(dense_tile16, "SLQ_DENSE_TILE16", 0, "keep the 16-row dense kernel also for wide panels")                                                     \
  PLAN(dense_lds, "SLQ_DENSE_LDS", 1, "fp64 dense product with the operands staged in LDS (0: k_dense_mfma_tile)")                                   \
  PLAN(dense_ksplit, "SLQ_DENSE_KSPLIT", 0, "K split of the big-tile dense kernels (0: fewest workgroup rounds)")                                    \
  PLAN(pipe, "SLQ_PIPE", -1, "pipelined row loop in the dots/update passes (-1: by operator)")                                                       \
  PLAN(lpr, "SLQ_LPR", 0, "lanes per row, 8/16/32/64 (0: by the number of probes)")                                                                  \
  PLAN(blocks_per_cu, "SLQ_BLOCKS_PER_CU", kAuto, "resident workgroups per CU: SpMM and streaming sweeps (auto: 4 / 2)")                             \
  PLAN(blocks_per_cu_spmm, "SLQ_BLOCKS_PER_CU_SPMM", kAuto, "... of k_spmm_3term alone")                                                            \
  PLAN(blocks_per_cu_stream, "SLQ_BLOCKS_PER_CU_STREAM", kAuto, "... of the streaming sweeps alone")                                                \
  PLAN(blocks_per_cu_fused, "SLQ_BLOCKS_PER_CU_FUSED", kAuto, "... of the dots/update passes, per panel (auto: 2; 1 with the pipelined loop)")       \
  PLAN(blocks_per_cu_alpha, "SLQ_BLOCKS_PER_CU_ALPHA", 0, "... of the alpha pass, total over the panels (0: by gathers per row)")                    \
  PLAN(blocks_per_cu_tiled, "SLQ_BLOCKS_PER_CU_TILED", kAuto, "... of the barrier-tile passes (auto: what their LDS images admit)")                  \
  PLAN(tiled_wgs_per_xcd, "SLQ_TILED_WGS_PER_XCD", kAuto, "experiments: fewer workgroups sweeping each XCD chunk in the tiled passes")               \
  PLAN(alpha_lds_pad, "SLQ_ALPHA_LDS_PAD", kAuto, "LDS padding (bytes) that caps the alpha pass's residency (auto: 0 or 65536)")                     \
  PLAN(fused_pad, "SLQ_FUSED_LDS_PAD", -1, "... of the dots/update passes (-1: by row loop)")                                                        \
  PLAN(spmm_pad, "SLQ_SPMM_LDS_PAD", 57344, "... of k_spmm_3term")                                                                                   \
  PLAN(known_norm, "SLQ_KNOWN_NORM", 1, "Rademacher probes drawn on the device skip the norm sweep (it is n)")                                       \
  PLAN(pinned_upload, "SLQ_PINNED_UPLOAD", 1, "slq_plan_set_probes through two pinned buffers (0: direct copy)")                                     \
  PLAN(debug_pass, "SLQ_DEBUG_PASS", 3, "diagnostic builds: the pass (PASS_* code) whose time line is stamped")

// *present: the variable exists, empty or not (SLQ_TILES: "set" lowers the size from which tiles are tried)
inline int env_int(const char *name, int dflt, bool *present = nullptr) {
  const char *s = getenv(name);
  if (present) *present = s != nullptr;
  return (s && *s) ? atoi(s) : dflt;
}
inline int or_auto(int v, int dflt) { return v != kAuto ? v : dflt; }

#define SLQ_SW_FIELD(field, name, dflt, meaning) int field = dflt;
#define SLQ_SW_READ(field, name, dflt, meaning) s.field = env_int(name, dflt);
#define SLQ_SW_NONE(field, name, dflt, meaning)

struct OperatorSwitches {
  SLQ_SWITCH_TABLE(SLQ_SW_FIELD, SLQ_SW_NONE, SLQ_SW_FIELD, SLQ_SW_NONE)
  bool tiles_forced = false;  // SLQ_TILES was set at all
};
struct PlanSwitches {
  SLQ_SWITCH_TABLE(SLQ_SW_NONE, SLQ_SW_FIELD, SLQ_SW_FIELD, SLQ_SW_NONE)
};

#define SLQ_SW_TILES_FORCED(field, name, dflt, meaning) env_int(name, dflt, &s.tiles_forced);
inline OperatorSwitches read_operator_switches() {
  OperatorSwitches s;
  SLQ_SWITCH_TABLE(SLQ_SW_READ, SLQ_SW_NONE, SLQ_SW_READ, SLQ_SW_NONE)
  SLQ_SWITCH_TABLE(SLQ_SW_NONE, SLQ_SW_NONE, SLQ_SW_TILES_FORCED, SLQ_SW_NONE)
  return s;
}
inline PlanSwitches read_plan_switches() {
  PlanSwitches s;
  SLQ_SWITCH_TABLE(SLQ_SW_NONE, SLQ_SW_READ, SLQ_SW_READ, SLQ_SW_NONE)
  s.omega = s.omega < 0 ? 0 : (s.omega > 2 ? 2 : s.omega);
  return s;
}
#define SLQ_SW_USE(field, name, dflt, meaning) inline int read_##field() { return env_int(name, dflt); }
SLQ_SWITCH_TABLE(SLQ_SW_NONE, SLQ_SW_NONE, SLQ_SW_NONE, SLQ_SW_USE)

#undef SLQ_SW_FIELD
#undef SLQ_SW_READ
#undef SLQ_SW_NONE
#undef SLQ_SW_TILES_FORCED
#undef SLQ_SW_USE

}  // namespace slq
