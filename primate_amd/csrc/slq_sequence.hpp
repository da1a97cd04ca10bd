// slq_sequence.hpp — what one Lanczos step launches, as a value. Plain C++ (no HIP include): pure integer and boolean logic over
// the facts of a plan and its operator, so that it runs without a device (slq_debug_step_shape, tests/test_sequence_cpu.py).
// enqueue_run (slq.hip) asks step_shape() once per step and launches what the answer says; slq_plan_describe reports
// plan_sequence_of(), which is computed from the same answer.
#pragma once

#include <algorithm>

namespace slq {
namespace seq {

constexpr int kMaxFusedR = 8;  // == kFusedMaxR (slq_common.hpp; slq.hip asserts the equality)
constexpr int kMaxRingR = 3;   // == kRingMaxR

// What the decision depends on. The first block is given (operator, plan geometry, switches as read when the plan was created:
// slq_switches.hpp); the second is derived from it by derive_plan_flags() exactly once, when the plan is created.
struct SequenceFacts {
  // operator
  int csr = 0;           // a CSR operator (every other kind takes the sweeps)
  int far_le4 = 0;       // far_per_row <= 4: the gathers are served from cache
  int tiles_ringed = 0;  // the operator's tiles are built to the caps of the ring-fed kernels
  int upper = 0;         // exactly symmetric: it has the upper-triangle copy (slq_operator::upper)
  // plan
  int ringR = 0;         // panel rows per wave instruction of the tile stream the plan uses (0: the plan uses no tiles)
  int rs_desc_u = 0;     // the plan's ring-fed alpha pass has an upper-triangle stream
  int rs_u_padded = 0;   // ... whose rows are padded to whole chunks
  int deg = 0, orth = 0, nstale = 0;
  int basis_mode = 0;    // 0 ring only, 1 kept basis, 2 recompute
  int dense_class = 0;   // the dense kernel id (slq_plan_dense_path); >= 2: the matrix-core product with its three-term epilogue
  int pipelined = 0;     // the generic dots/update passes run the pipelined row loop
  int omega_on = 0;      // the plan offers its full windows to the edge recurrence
  // switches
  int fused = 1, merged = 1, mgs = 0, stored_u = 1, nt = 1, cross = 1, sw_gram = 1, sw_gram_csr = 1, sw_ring_gen = 1, sw_ring_deep = 1,
      last_store = 0, ring_alpha = 2, ring_rev = 1;
  // derived (derive_plan_flags)
  int ring_gen = 0;      // every ring-fed pass of the plan runs k_ring_pass (always for ringR > 1)
  int ring_deep = 0;     // steps with 4..8 ring columns run k_ring_pass with 8 waves (else the generic passes)
  int gram = 0;          // ring-fed plans: steps with 1..8 ring columns take their projections from Gram rows
  int gram_csr = 0;      // ... also where the plan's fused passes are the generic ones
  int last_nostore = 0;  // the update pass of a run's last step does not store W_deg
};
constexpr int kNumFacts = 27;  // the given ones, in the order of facts_from_array

inline void derive_plan_flags(SequenceFacts &f) {
  const bool ringed_plan = f.ringR > 0 && f.tiles_ringed;
  f.ring_gen = ringed_plan && (f.ringR > 1 || (f.nt && f.sw_ring_gen));
  f.ring_deep = ringed_plan && (f.ringR > 1 || f.nt) && f.sw_ring_deep;
  // the Gram sequence needs every step of the window on k_ring_pass, i.e. the deep form too, and an EXACTLY symmetric operator
  f.gram = f.ring_gen && f.ring_deep && f.merged && !f.mgs && f.upper && f.sw_gram;
  f.gram_csr = f.csr && f.ringR == 0 && f.upper && f.merged && !f.mgs && f.nt && f.sw_gram && f.sw_gram_csr;
  f.last_nostore = f.last_store == 0;
}

inline SequenceFacts facts_from_array(const int *a) {
  SequenceFacts f;
  int *const given[kNumFacts] = {&f.csr, &f.far_le4, &f.tiles_ringed, &f.upper, &f.ringR, &f.rs_desc_u, &f.rs_u_padded, &f.deg, &f.orth, &f.nstale,
                                 &f.basis_mode, &f.dense_class, &f.pipelined, &f.omega_on, &f.fused, &f.merged, &f.mgs, &f.stored_u, &f.nt, &f.cross,
                                 &f.sw_gram, &f.sw_gram_csr, &f.sw_ring_gen, &f.sw_ring_deep, &f.last_store, &f.ring_alpha, &f.ring_rev};
  for (int i = 0; i < kNumFacts; ++i) *given[i] = a[i];
  f.tiles_ringed = a[2] == 2;  // (given as the operator's tiles: 0 none, 1 landed behind barriers, 2 ring-fed)
  derive_plan_flags(f);
  return f;
}

// the sequences a step can take
enum Sequence {
  SEQ_GRAM_RING = 0,     // ring-fed Gram: alpha-only pass, k_fin_gram, (rescue pair), k_ring_pass<UPDATEG>, k_fin_beta_gram
  SEQ_GRAM_CSR = 1,      // the same on the generic passes (k_csr_pass<PASS_UPDATEG>)
  SEQ_MERGED = 2,        // fused passes: alpha+dots pass, update pass
  SEQ_SEPARATE = 3,      // fused passes: alpha pass, dots pass (r > 0), update pass
  SEQ_STORED_U = 4,      // the merged sequence whose first pass stores u for the update pass to read back
  SEQ_SWEEPS_CGS = 5,    // store-and-revisit sweeps, block classical Gram-Schmidt
  SEQ_SWEEPS_MGS = 6,    // ... exact modified Gram-Schmidt order, one column at a time
  SEQ_SWEEPS_PLAIN = 7   // ... no reorthogonalisation (r == 0)
};
// the product of the sweeps' first launch
enum SweepProduct { PRODUCT_RING = 0, PRODUCT_CSR = 1, PRODUCT_DENSE = 2, PRODUCT_UNFUSED = 3 };
// the grid whose partials a finalize kernel reduces
enum Blocks { BLK_A = 0, BLK_S = 1, BLK_U = 2, BLK_T = 3, BLK_F = 4, BLK_DENSE = 5 /* what launch_dense_mfma reports */ };

// Everything the launch code needs for step j.
struct StepShape {
  int seq = SEQ_SWEEPS_PLAIN;
  int r = 0;               // reorth columns: the last `orth` ring vectors (before step orth-1 only j+1 exist, plus stale ones)
  int tiled = 0;           // the dots/update passes run on the plan's tiles
  int gen = 0;             // ... through k_ring_pass rather than k_csr_ring_pass
  int alpha_tiled = 0;     // the alpha-only pass runs on the tiles
  int alpha_upper = 0;     // ... ring-fed over the upper-triangle stream
  int half = 0;            // the generic alpha-only pass walks the upper-triangle copy
  int pipe_on = 0;         // pipelined row loop in the generic dots/update passes
  int xt_alpha = 0;        // complete xt word of the alpha-only pass: bit 0 W_p left unread, bit 3 padded rows
  int xt_dots = 0;         // ... of the dots / alpha+dots pass: bit 1 stores u
  int xt_update = 0;       // ... of the update pass: bit 0 cross term, bit 1 reads u, bit 2 reverse sweep, bit 4 (16) stores nothing
  int omega = 0;           // the window is offered to the edge recurrence
  int est_prev = 0;        // ... which has a previous estimate (step 2 is the first with a full window)
  int product = PRODUCT_UNFUSED;  // sweeps: which kernel forms A W_j
  int blk_alpha = BLK_S;   // the grid behind the alpha partials (k_fin_alpha, k_fin_gram)
  int blk_dots = BLK_S;    // ... behind the dots partials (k_fin_adots, k_fin_gamma)
  int blk_beta = BLK_S;    // ... behind the norm partials (k_fin_beta, k_fin_beta_gram)
  int prev_xt = 0;         // out: this step's update pass leaves the cross term W_{j+1}.W_j behind
};
constexpr int kNumShape = 18;

inline void shape_to_array(const StepShape &s, int *out) {
  const int v[kNumShape] = {s.seq, s.r, s.tiled, s.gen, s.alpha_tiled, s.alpha_upper, s.half, s.pipe_on, s.xt_alpha, s.xt_dots, s.xt_update, s.omega,
                            s.est_prev, s.product, s.blk_alpha, s.blk_dots, s.blk_beta, s.prev_xt};
  for (int i = 0; i < kNumShape; ++i) out[i] = v[i];
}

inline StepShape step_shape(const SequenceFacts &f, int j, bool prev_xt) {
  StepShape s;
  s.r = f.orth > 0 ? std::min(j + 1 + f.nstale, f.orth) : 0;
  const int r = s.r;
  // exact modified Gram-Schmidt order (one ring column at a time, each dot taken on the updated w): used when stale ring
  // columns take part, whose projections are NOT small, so block-CGS and the reference's MGS would differ at second order
  const bool mgs = f.nstale > 0 || f.mgs;
  // Recomputing the SpMM in every pass pays while the gathers are served from cache; where a row's neighbours are scattered
  // over the whole vector the sweeps that gather once and store are faster. fused == 2 forces the passes.
  const bool gathers_cached = f.fused == 2 || f.far_le4;
  const bool plan_tiled = f.ringR > 0;
  // ... with r >= 1 the merged pass can store u for the update pass to read back: one gather pass per step
  const bool stored_u = f.csr && f.fused != 0 && !gathers_cached && r >= 1 && r <= kMaxFusedR && !mgs && f.stored_u && f.merged && !plan_tiled;
  if (!(f.csr && f.fused != 0 && (gathers_cached || stored_u) && r <= kMaxFusedR && !mgs)) {
    // ---- store-and-revisit sweeps ----
    s.seq = r == 0 ? SEQ_SWEEPS_PLAIN : (mgs ? SEQ_SWEEPS_MGS : SEQ_SWEEPS_CGS);
    if (f.csr && plan_tiled && f.tiles_ringed) s.product = PRODUCT_RING, s.gen = f.ring_gen, s.blk_alpha = BLK_T;
    else if (f.csr) s.product = PRODUCT_CSR, s.blk_alpha = BLK_A;
    else if (f.dense_class >= 2) s.product = PRODUCT_DENSE, s.blk_alpha = BLK_DENSE;
    else s.product = PRODUCT_UNFUSED, s.blk_alpha = BLK_S;
    return s;
  }
  // ---- fused passes: recompute the SpMM, write once ----
  // ring-sized tiles serve up to kMaxRingR ring columns; steps with more take the deep form or the generic passes, on the same row order
  const bool tiled = plan_tiled && !stored_u && (!f.tiles_ringed || r <= kMaxRingR || f.ring_deep);
  const bool gen = tiled && f.tiles_ringed && (f.ring_gen || r > kMaxRingR);
  // the alpha-only pass of a symmetric operator: ring-fed over the upper-triangle stream where the plan has one (ring_alpha 2;
  // else the generic upper-triangle pass), ring-fed over the full rows (1), generic (0)
  const bool alpha_tiled = tiled && !(f.tiles_ringed && f.upper && (f.ring_alpha == 0 || (f.ring_alpha == 2 && !f.rs_desc_u)));
  s.tiled = tiled, s.gen = gen, s.alpha_tiled = alpha_tiled;
  s.alpha_upper = alpha_tiled && f.tiles_ringed && f.rs_desc_u && f.ring_alpha == 2;
  s.half = !alpha_tiled && f.upper;
  s.pipe_on = f.pipelined && !tiled;
  const int blk_tu = tiled ? BLK_T : BLK_U;
  s.blk_alpha = alpha_tiled ? BLK_T : BLK_F;
  s.blk_dots = s.blk_beta = blk_tu;
  const int pad_bit = (alpha_tiled && gen && s.alpha_upper && f.rs_u_padded) ? 8 : 0;
  const int rev_bit = (tiled && f.tiles_ringed && f.ring_rev) ? 4 : 0;
  // the LAST step of a run whose basis is not kept stores nothing: W_deg is never read. Not the stored-u sequence, nor the
  // kernels of the barrier tiles and k_csr_ring_pass, which have no such form.
  const int nostore_bit = (j == f.deg - 1 && f.basis_mode != 1 && f.last_nostore && !stored_u && (!tiled || gen)) ? 16 : 0;
  // r >= 1: alpha comes out of the dots pass (the tiled kernels have the merged form only)
  const bool merged = r > 0 && (tiled || f.merged);
  const bool gram_ring = gen && f.gram && r >= 1;
  const bool gram_csr = f.gram_csr && !tiled && gathers_cached && !stored_u && r >= 1;
  if (gram_ring || gram_csr) {
    s.seq = gram_ring ? SEQ_GRAM_RING : SEQ_GRAM_CSR;
    s.xt_alpha = (j > 0 ? 1 : 0) | pad_bit;  // (alpha_j's -beta q_j.q_{j-1} part is a Gram entry: the pass leaves W_p unread)
    s.xt_update = rev_bit | nostore_bit;
    s.omega = gram_ring && f.omega_on && r == 3 && f.orth == 3;
    s.est_prev = s.omega && j >= 3;
    return s;
  }
  const int su = stored_u ? 2 : 0;
  const int cross_bit = (!merged && f.cross) ? 1 : 0;
  s.seq = stored_u ? SEQ_STORED_U : (merged ? SEQ_MERGED : SEQ_SEPARATE);
  s.xt_alpha = ((prev_xt && j > 0) ? 1 : 0) | pad_bit;  // cross term: the previous update pass left W_c.W_p behind, so the alpha pass skips W_p
  s.xt_dots = merged ? su : 0;
  s.xt_update = cross_bit | su | rev_bit | nostore_bit;
  s.prev_xt = cross_bit;
  return s;
}

// which launch sequence the steps with r <= kMaxFusedR take (slq_plan_describe): 0 sweeps, 1 recompute passes, 2 stored u,
// 4 Gram. Step 0 is such a step of every plan (r = min(1 + nstale, orth)).
inline int plan_sequence_of(const SequenceFacts &f) {
  switch (step_shape(f, 0, false).seq) {
    case SEQ_GRAM_RING: case SEQ_GRAM_CSR: return 4;
    case SEQ_MERGED: case SEQ_SEPARATE: return 1;
    case SEQ_STORED_U: return 2;
    default: return 0;
  }
}

// ---- the closing tail ("the closing tail") ------------------------------------------------------------
// The update pass of a run's last step, j = deg - 1, and the scalar kernel behind it (k_fin_beta_gram / k_fin_beta) produce
// beta_deg, a Gram row, the next sc / cp, the stop rule's flags and the edge recurrence's counters of that step: no quadrature
// reads any of them (k_quadrature: alpha[0 .. deg), nu[1 .. deg)). Where that pass also stores nothing, a run that reaches deg
// leaves both launches out and the plan launches them when an entry first asks for what they write (slq.hip:
// flush_closing_tail). A step can be launched in these two parts:
enum StepPart { STEP_FRONT = 1, STEP_TAIL = 2, STEP_WHOLE = 3 };
// A plan has a lazy tail where its closing update pass carries the no-store bit and the plan is a plain quadrature plan
// (basis_mode 0: a recompute plan's runs, forward and replay, stay whole). lazy_close: the plan was not created under
// SLQ_LAST_STORE=2, which keeps the pass in the run. values_fixed: nothing rewrites the operator's values under a live plan - a
// deferred pass reads the CSR again, so the plans of an affine operator A + t B (slq_operator_set_parameter rewrites its values
// in place) stay whole: their beta_deg must be that of the t the run saw. Stale ring columns put every step on the sweeps, which
// have no such bit.
inline bool has_lazy_tail(const SequenceFacts &f, int lazy_close, int values_fixed) {
  if (!lazy_close || !values_fixed || f.deg < 1 || f.basis_mode != 0) return false;
  return (step_shape(f, f.deg - 1, false).xt_update & 16) != 0;
}

// ---- Chebyshev runs (slq_cheb.hpp) ----------------------------------------------------------------
// A Chebyshev step w_{j+1} = 2 A~ w_j - w_{j-1} IS the update pass of the orth-0 Lanczos step with constant coefficients:
// no alpha pass, no dots pass. What it launches is therefore read off step_shape's answer for the same facts at orth = 0 (deg =
// the number of Chebyshev steps), so that a plan takes the same kernels for both kinds of run.
struct ChebStepShape {
  int sweeps = 1;          // 1: product kernel, then k_cheb_axpy (k_cheb_3term after an unfused product); 0: one fused update pass
  int tiled = 0;           // the update pass runs on the plan's tiles
  int gen = 0;             // ... through k_ring_pass (fused), or the sweeps' ring product through it
  int pipe_on = 0;         // pipelined row loop in the generic update pass
  int xt_update = 1;       // complete xt word of the update pass: bit 0 cross term (always), bit 2 reverse sweep, bit 4 (16) stores nothing
  int product = PRODUCT_UNFUSED;  // sweeps: which kernel forms A W_j
  int blk_product = BLK_S; // sweeps: the grid of the product kernel (its alpha partials are not read)
  int blk = BLK_S;         // the grid behind the norm and cross partials k_fin_cheb reduces
  int alpha_pass = 0;      // always 0: a Chebyshev step has no alpha pass
};
constexpr int kNumChebShape = 9;

inline void cheb_shape_to_array(const ChebStepShape &s, int *out) {
  const int v[kNumChebShape] = {s.sweeps, s.tiled, s.gen, s.pipe_on, s.xt_update, s.product, s.blk_product, s.blk, s.alpha_pass};
  for (int i = 0; i < kNumChebShape; ++i) out[i] = v[i];
}

inline ChebStepShape cheb_step_shape(const SequenceFacts &facts, int j) {
  SequenceFacts f = facts;
  f.orth = 0, f.nstale = 0;
  const StepShape l = step_shape(f, j, false);
  ChebStepShape s;
  if (l.seq == SEQ_SWEEPS_PLAIN) {
    s.sweeps = 1, s.gen = l.gen, s.product = l.product, s.blk_product = l.blk_alpha;
    s.blk = BLK_S;  // (k_cheb_axpy / k_cheb_3term run on the streaming grid, as k_axpy_norm does)
    s.xt_update = 1;
    return s;
  }
  // (orth = 0 leaves SEQ_SEPARATE only: r = 0 rules out the merged, stored-u and Gram sequences)
  s.sweeps = 0, s.tiled = l.tiled, s.gen = l.gen, s.pipe_on = l.pipe_on, s.blk = l.blk_beta;
  s.xt_update = l.xt_update | 1;  // the cross term is a moment: always reduced, whatever SLQ_CROSS says
  return s;
}

// ---- the action of a Chebyshev run (k_cheb_accumulate) ---------------------------------------------
// Y = sum_{k <= nsteps} c_k w_k is summed while the w_k pass through the ring: w_t lives in slot t mod S, step j reads w_j and
// w_{j-1} and writes w_{j+1}, a FINISHED vector (unlike the Lanczos residual), and w_0 - the probes - is column 0 of the first
// piece: no stash panel. An accumulation launch is issued after step j when `acc` columns c0 .. j+1 are unconsumed, or after
// the last step, and consumes them all. Step j + 1 then writes slot (j + 2) mod S, which must hold a consumed column and neither
// w_{j+1} nor w_j: before that step at most acc - 1 columns c0 .. j+1 are unconsumed, so S = acc slots suffice (with acc - 1
// the step that finishes the acc-th unconsumed column would overwrite column c0), and a run of fewer than acc columns keeps
// them all: S = nsteps + 1. An action plan's steps are cheb_step_shape's with the fact last_store = 1: w_nsteps is read.
inline int cheb_action_ring_slots(int nsteps, int acc) { return std::max(2, std::min(acc, nsteps + 1)); }

// the piece issued after step j, given that columns c0 .. j+1 are unconsumed: its number of columns, 0 for none
inline int cheb_action_piece_after(int nsteps, int acc, int j, int c0) {
  const int unconsumed = j + 2 - c0;
  return (unconsumed >= acc || j == nsteps - 1) ? unconsumed : 0;
}

// every piece of a run in launch order: t0[i], nc[i] (the first cap of them; either may be null), after[i] the step it follows.
// Returns the number of pieces.
inline int cheb_action_schedule(int nsteps, int acc, int *t0, int *nc, int *after, int cap) {
  int np = 0, c0 = 0;
  for (int j = 0; j < nsteps; ++j) {
    const int m = cheb_action_piece_after(nsteps, acc, j, c0);
    if (!m) continue;
    if (np < cap) {
      if (t0) t0[np] = c0;
      if (nc) nc[np] = m;
      if (after) after[np] = j;
    }
    ++np;
    c0 += m;
  }
  return np;
}

}  // namespace seq
}  // namespace slq
