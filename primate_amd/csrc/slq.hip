// slq.hip — C-ABI implementation (include/slq.h) over the kernels in slq_kernels.hpp.
// Host logic only: handles, workspace, launch sequencing, HIP-event profiling.
// Built with: hipcc --offload-arch=gfx950 -O3 -shared -fPIC (see __graft_entry__.build()).
#include "../../include/slq.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <atomic>
#include <mutex>
#include <new>
#include <string>
#include <system_error>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "slq_kernels.hpp"
#include "slq_ring_api.h"
#include "slq_ring.hpp"  // (RingGeo constants: no kernel of it is instantiated here)
#include "slq_build.hpp"  // an operator's derived data built on the device
#include "slq_density.hpp"  // spectral density accumulator (slq_density_*)
#include "slq_radau.hpp"    // prefix quadrature, Gauss-Radau rule, stage statistics (slq_plan_quadrature_at)
#include "slq_action.hpp"   // two-pass f(A)v: the accumulation of a recompute plan's replay (slq_plan_create_recompute)
#include "slq_switches.hpp"  // the table of run-time switches, OperatorSwitches, PlanSwitches
#include "slq_sequence.hpp"  // what a step launches, as a value (step_shape)
#include "slq_layout.hpp"    // an operator's layout as a value and the host analysis behind it (layout_prefilter, decide_layout)
#include "slq_plan_shape.hpp"  // what creating a plan decides, as a value (plan_shape)
#include "slq_cheb.hpp"      // Chebyshev moments: the kernels of slq_plan_run_chebyshev, _moment_sum, slq_density_update_moments
#include "slq_sddmm.hpp"     // sampled dense-dense product on a CSR pattern: schedule (sddmm_schedule) and kernel of slq_sddmm_*
#include "slq_kernelop.hpp"  // matrix-free kernel operator (slq_kernel_*): validation, schedule, k_kernel_rescale, k_kernel_panel
#include "slq_kernelgrad.hpp"  // hyperparameter gradients of the kernel operator (slq_kernel_grad_*): schedule, k_kernel_grad, k_kernel_grad_sum
#include "slq_kernelcross.hpp"  // cross-covariance products (slq_kernel_cross_*): schedule, the launch functions of slq_kernelcross.hip
#include "slq_kernelfeature.hpp"  // random Fourier features (slq_kernel_feature_*): schedule, the launch function of slq_kernelfeature.hip
#include "slq_kernelfeatureadj.hpp"  // their adjoint (slq_kernel_feature_rmatmat / _rdmat): schedule, the launch function of slq_kernelfeatureadj.hip
#include "slq_kernelpointgrad.hpp"  // gradients in the points (slq_kernel_pointgrad_*): schedule, the launch functions of slq_kernelpointgrad.hip
#include "slq_toeplitz.hpp"  // the Toeplitz operator (slq_toeplitz_*): pass structure, host symbol transform, the launch functions of slq_toeplitz.hip
#include "slq_operator.hpp"  // the operator handle and the values it owns (DevBuf, CsrArrays, TileStream, KernelPoints)

using namespace slq;

// ---------------------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------------------
static thread_local char g_err[1024] = "";

static int fail(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess)                                                                      \
      return fail(_e == hipErrorOutOfMemory ? SLQ_ENOMEM : SLQ_EHIP, "%s failed: %s (%s:%d)",  \
                  #expr, hipGetErrorString(_e), __FILE__, __LINE__);                           \
  } while (0)

#define SLQ_TRY(expr)           \
  do {                          \
    int _rc = (expr);           \
    if (_rc != SLQ_OK) return _rc; \
  } while (0)

extern "C" const char *slq_last_error(void) { return g_err; }
extern "C" int slq_version(void) { return SLQ_VERSION; }

// ---------------------------------------------------------------------------------------------------
// handles
// ---------------------------------------------------------------------------------------------------
struct slq_context {
  int device;
  hipStream_t stream;
  bool own_stream;
  int num_cus;
  // Operators, plans, diag accumulators and device matrices hold the context they were created on. A context
  // destroyed while such objects are alive (a garbage collector tears handles down in no particular order) only
  // becomes unusable for NEW objects; its stream lives until the last dependant has been destroyed.
  int refs = 0;
  bool dead = false;
  // pinned staging ring for host -> device uploads of probes (slq_plan_set_probes): two buffers, so that the host-side copy
  // of one chunk runs while the previous chunk is on its way over PCIe
  void *pin[2] = {nullptr, nullptr};
  hipEvent_t pin_ev[2] = {nullptr, nullptr};
  bool pin_busy[2] = {false, false};
  size_t pin_bytes = 0;
};
static void ctx_retain(slq_context *ctx) { ++ctx->refs; }
static void ctx_free(slq_context *ctx) {
  hipSetDevice(ctx->device);
  for (int b = 0; b < 2; ++b) {
    if (ctx->pin[b]) hipHostFree(ctx->pin[b]);
    if (ctx->pin_ev[b]) hipEventDestroy(ctx->pin_ev[b]);
  }
  if (ctx->own_stream) hipStreamDestroy(ctx->stream);
  delete ctx;
}
static void ctx_release(slq_context *ctx) {
  if (--ctx->refs == 0 && ctx->dead) ctx_free(ctx);
}
// The end of every side object (accumulators, cross objects, feature maps, device matrices): a struct that holds `slq_context *ctx`
// and owns its device arrays as DevBuf members. Work queued on the stream may still read those arrays, so the stream is waited for
// before they go. (slq_diag and slq_density did not wait explicitly before their arrays became DevBufs: their hipFree waited for the
// device, so nothing observable has changed.)
template <typename H> static int handle_destroy(H *h) {
  if (!h) return SLQ_OK;
  hipSetDevice(h->ctx->device);
  hipStreamSynchronize(h->ctx->stream);
  slq_context *ctx = h->ctx;
  delete h;
  ctx_release(ctx);
  return SLQ_OK;
}
// b holds at least `need` bytes: the one way a scratch, staging or column buffer grows (what it held is gone; it never shrinks)
static int devbuf_grow(DevBuf &b, size_t need, const char *who, const char *what = "scratch") {
  if (b.bytes() >= need) return SLQ_OK;
  const hipError_t e = b.alloc(need);
  if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? SLQ_ENOMEM : SLQ_EHIP, "%s: %s of %zu bytes: %s", who, what, need, hipGetErrorString(e));
  return SLQ_OK;
}

// (OP_CSR .. OP_KERNEL, the kinds of an operator: slq_plan_shape.hpp)
static_assert(kF32 == SLQ_F32 && kF64 == SLQ_F64, "slq_plan_shape.hpp: the dtype codes of include/slq.h");

// (slq_operator, the handle of an operator, and the values it owns - DevBuf, CsrArrays, TileStream, KernelPoints: slq_operator.hpp)

struct ProfEvent {
  hipEvent_t a, b;
  int kind;
};

struct slq_plan {
  slq_context *ctx;
  slq_operator *op;
  int dtype, n, nprobes, deg, orth, keep_basis;
  int LPR, PW, NP, bpad, S;
  size_t esz;
  int64_t slot_stride;  // elements between ring slots
  void *ring;
  void *T;              // product panel for dense / callback / Gram operators
  void *T2;             // Gram operator: the intermediate A W_c (mrows rows per panel)
  void *stage;          // column-major staging (probe upload, callback round trips)
  int stage_cols;
  StepState st;
  double *scal;         // one allocation behind all StepState arrays
  double *part;
  int nblkA, nblkS, nblkU, nblkT;  // grids: SpMM, streaming sweeps, fused dots/update passes, tiled passes
  int nblkF;                       // grid of the fused alpha pass
  size_t alpha_pad;                // LDS padding that caps its residency
  double *quad_d, *nodes_d, *weights_d;
  int *fail_d;
  int *ring_fail_d;
  // the Gauss rule of the last run in nodes_d / weights_d: 0 not computed yet, 1 by slq_plan_quadrature (QL status in
  // rule_fail_h), 2 by slq_density_update (QL status in the device word fail_d[2]); a run resets it to 0
  int rule_src = 0;
  int rule_fail_h = 0;
  int rmax;
  bool probes_ready, ran;
  int pdf_sphere;
  bool prof;
  std::vector<ProfEvent> events;
  std::vector<ProfEvent> pool;
  slq_profile acc;
  std::vector<char> hbuf;  // host staging for callback operators
  int nstale;                 // > 0: the reorthogonalisation also sees nstale preloaded vectors t = -1 .. -nstale
  // the launch sequence of steps [j0, j1) captured once per (j0, j1, rtol, variant); the one-shot run is the entry (0, deg).
  // Everything else the sequence depends on is fixed when the plan is created (PlanSwitches), so variant is what can change
  // under a live plan: the number of stale ring columns (slq_debug_plan_mark_stale).
  struct GraphEntry {
    int j0, j1;
    double rtol;
    unsigned variant;  // (graph_variant: nstale, and the top bit for a kernel operator with a diagonal scale)
    hipGraphExec_t exec;
    bool xt_out;  // prev_xt after step j1 - 1
  };
  std::vector<GraphEntry> graphs;  // (at most kGraphCacheMax: the oldest entry leaves first)
  // resumable runs (slq_plan_run_steps): steps done since the probes were set, the rtol the run began with, and the one
  // piece of host state a step hands to the next - the previous update pass produced the cross term W_j.W_{j-1}
  int cur = 0;
  double run_rtol = 0.0;
  bool prev_xt = false;
  // the closing tail (slq_sequence.hpp: has_lazy_tail): a run that reached deg left the update pass of step
  // deg - 1 and its scalar kernel out; what they need to be launched later (flush_closing_tail). New probes drop it.
  struct ClosingTail {
    bool pending = false;
    int j = 0;             // the step: deg - 1
    double rtol = 0.0;     // the run's rtol (the stop rule of k_fin_beta / k_fin_beta_gram)
    seq::StepShape shape;  // the step as the run saw it: xt bits, grids, the edge recurrence's flags
  } closing;
  // slq_plan_quadrature_at (allocated by its first call): quad | gauss | stage[4] | nodes | weights (P x (deg + 1) each), two flag words
  double *at_d = nullptr;
  int *at_flags = nullptr;
  PlanSwitches sw;            // the switches as they were when the plan was created (slq_switches.hpp)
  bool pipelined;             // dots/update passes run the pipelined row loop (slq_plan_create)
  int dense_ks;               // dense MFMA operator with big tiles: K split over this many workgroups per row tile (0: 16-row kernel)
  // ring-fed tile passes (k_csr_ring_pass / k_ring_pass): ringR = panel rows per wave instruction of the tile stream the plan
  // uses (0: no tiles; 1: the tiles as clustered, 1-KiB panel rows; 2, 4: merged tiles, 512-B / 256-B panel rows)
  int ringR;
  bool ring_gen;              // every ring-fed pass of the plan runs k_ring_pass (always for ringR > 1; SLQ_RING_GEN for ringR = 1)
  bool ring_deep;             // steps with 4..8 ring columns run k_ring_pass with 8 waves (SLQ_RING_DEEP; else the generic passes)
  bool gram;                  // steps with 1..8 ring columns take their projections from Gram rows of the update passes (SLQ_GRAM)
  bool gram_csr;              // ... also where the plan's fused passes are the generic ones (k_csr_pass<PASS_UPDATEG>: narrow panels, small operators; SLQ_GRAM_CSR, r04)
  // the operator's streams the plan's ring-fed passes read: full rows / upper triangle or null (their tile ranges and the upper
  // stream's padding are the shape's: rs_xcd, rs_xcd_u, rs_u_padded)
  const TileStream *rs_full = nullptr, *rs_upper = nullptr;
  bool ring_staged;          // the alpha-only pass's loaders go through registers (SLQ_RING_STAGED; slq_ring.hpp: GEO 1)
  int part_maxblk = 0;        // blocks per slab of `part`
  bool launch_error = false;  // a launcher declined (mis-dispatch): the run is invalid (enqueue_run)
  bool sweep_skip = true;     // the update sweep does not read ring columns whose coefficient is zero for every probe of the panel (SLQ_SWEEP_SKIP=0: reads them all)
  unsigned long long *sweep_cols_d = nullptr;  // {ring columns the update sweeps read, columns they were offered}, summed over launches and panels (slq_plan_sweep_columns)
  // the edge recurrence: state of the offered steps - D, rho, g3, Dm [bpad] each | read, rescue [deg + 1][NP] | counters
  bool omega_on = false;      // the plan offers its full-window steps (ring-fed Gram sequence, orth == 3, SLQ_OMEGA != 0)
  double *om_buf = nullptr;
  int *om_flags = nullptr;
  unsigned long long *om_cnt = nullptr;
  int *om_ticket = nullptr;   // [NP] tickets of k_omega_rescue_dot, zero between launches (beside the shape's regions: allocated with the plan where omega_on)
  int *om_census = nullptr;   // SLQ_OMEGA=2, any ring-fed Gram plan: non-zero gammas per step, window position and panel (slq_plan_window_census)
  double om_norm = 0.0;       // ||A||_inf of the operator when the plan was created
  bool last_nostore = true;   // the update pass of a run's last step does not store W_deg (plans without a kept basis; SLQ_LAST_STORE=1 stores)
  // two-pass f(A)v (slq_plan_create_recompute). basis_mode: 0 ring only, 1 kept basis, 2 recompute - the ring
  // has acc_cols + 1 slots at least, and two panels lie behind it: slot v_slot the stash of the probes, slot y_slot the output
  int basis_mode = 0;
  int acc_cols = 0;           // finished ring columns one accumulation launch consumes (<= kAccCols)
  int v_slot = 0, y_slot = 0; // where the action's probes and its output are (kept basis: slots 0 and deg)
  double *acc_coef = nullptr; // [deg][bpad] coefficients g_t of the action (st.gamma is live during the replay)
  bool stash_ready = false;   // the stash holds the probes of the last probe call ...
  bool stash_unit = false;    // ... which were device-drawn Rademacher probes taken with the known-norm shortcut
  bool acc_skip = true;       // the accumulation does not read columns whose coefficient is zero for every probe of the panel (SLQ_ACC_SKIP=0: reads them all)
  hipGraphExec_t replay_exec = nullptr;  // the replay (deg steps + accumulation launches: a linear chain) captured for replay_rtol / replay_variant
  double replay_rtol = 0.0;
  unsigned replay_variant = 0;  // (nstale, as GraphEntry::variant)
  bool replay_xt_out = false;
  // Chebyshev plan (slq_plan_create_chebyshev): deg is its number of steps, the geometry that of an orth-0 plan;
  // alpha / nu keep one row (nu_0), and there is no QL workspace
  bool cheb = false;
  bool cheb_ran = false;           // a Chebyshev run has been enqueued since the plan was created (its moments are those of the last run)
  double cheb_c = 0.0, cheb_h = 0.0;  // centre and half-width of the last run
  double *cheb_mu = nullptr;       // [2 deg + 1][bpad] moments
  int *cheb_out = nullptr;         // [bpad] outside flags
  double *cheb_coef = nullptr;     // [2 deg + 1] coefficients of slq_plan_moment_sum / damping factors of a density update | stage[4]
  // action plan (slq_plan_create_chebyshev_action): a ring of cheb_action_ring_slots slots, the output panel
  // y_slot behind it, every step stores (the fact last_store = 1), acc_cols = kChebAccCols
  bool cheb_action = false;
  // what the plan was created from and what creation decided (slq_plan_shape.hpp; the fields above that repeat shape values are
  // what the launchers read), and the device allocations of the shape's workspace table, by region
  PlanFacts facts;
  PlanShape shape;
  void *ws[kNumRegions] = {};
  uint64_t cheb_cols_read = 0, cheb_cols_offered = 0;  // ring columns its accumulation launches read / were offered (the mask is the host's)
};

// the entries of a Lanczos run are not for Chebyshev plans, and the other way round
static int need_lanczos(const slq_plan *p, const char *who) {
  if (p->cheb) return fail(SLQ_EINVAL, "%s: a Chebyshev plan has no Lanczos run (slq_plan_run_chebyshev, _get_moments, _moment_sum)", who);
  return SLQ_OK;
}
static int need_chebyshev(const slq_plan *p, const char *who) {
  if (!p->cheb) return fail(SLQ_EINVAL, "%s: not a Chebyshev plan (slq_plan_create_chebyshev)", who);
  return SLQ_OK;
}

// the closing tail of the last run (slq_plan::ClosingTail): launched by the entries that read what it writes, ...
static int flush_closing_tail(slq_plan *p);
// ... dropped, with no launch, by whatever replaces the probes: the ring slot it would read is about to be overwritten. `ran`
// is left to init_from_probes and run_range, as it always was.
static void drop_closing_tail(slq_plan *p) { p->closing.pending = false; }

// SLQ_TILES: 0 none, 1 workgroup tiles landed behind barriers (k_csr_tile_pass), 2 tiles fed through a ring of LDS slots by
// loader waves (k_csr_ring_pass). Read when an operator is created (the rows are regrouped into the tiles) and when a plan
// is created (whether its passes use them).
static_assert(OperatorSwitches{}.tiles == 2 && OperatorSwitches{}.tile_rows == kTileRows && OperatorSwitches{}.tile_cols == kTileCols, "slq_switches.hpp: tile defaults");
static_assert(seq::kMaxFusedR == kFusedMaxR && seq::kMaxRingR == kRingMaxR, "slq_sequence.hpp: the constants of slq_common.hpp");
static_assert(PlanSwitches{}.debug_pass == PASS_ADOTS, "slq_switches.hpp: SLQ_DEBUG_PASS");
// the edge recurrence's certificate: a step adds kOmegaC eps_F ||A||_inf to the noise radius (8x the largest
// one-step innovation the verify mode has seen on the device, and not less than 1); a zero is certified below orth_tol / kOmegaKappa
constexpr double kOmegaC = 3.5;
constexpr double kOmegaKappa = 4.0;
static_assert(PlanSwitches{}.ring_alpha_max_x100 == (int)(100 * kTileAlphaColsPerRow), "slq_switches.hpp: SLQ_RING_ALPHA_MAX_X100");

// Host-to-device copies of an operator's arrays, run by helper threads while the caller builds the next arrays: a copy from
// pageable memory blocks its caller at ~10 GB/s, 40 of the 160 ms a 10^6-row operator took to create. Every source must
// outlive wait() (declare the queue AFTER the buffers it reads: its destructor joins first).
struct UploadQueue {
  struct Job { void *dst; const void *src; size_t bytes; };
  int device;
  std::vector<std::thread> th;
  std::mutex m;
  hipError_t err = hipSuccess;
  explicit UploadQueue(int dev) : device(dev) {}
  void push(std::vector<Job> jobs) {
    auto run = [this](const std::vector<Job> &js) {
      hipError_t e = hipSetDevice(device);
      for (const Job &j : js)
        if (e == hipSuccess && j.bytes) e = hipMemcpy(j.dst, j.src, j.bytes, hipMemcpyHostToDevice);
      if (e != hipSuccess) {
        std::lock_guard<std::mutex> g(m);
        if (err == hipSuccess) err = e;
      }
    };
    try {
      th.emplace_back([run, jobs]() { run(jobs); });
    } catch (const std::system_error &) {  // no thread to be had: the caller copies
      run(jobs);
    }
  }
  hipError_t wait() {
    for (auto &t : th)
      if (t.joinable()) t.join();
    th.clear();
    return err;
  }
  ~UploadQueue() { wait(); }
};

// ---------------------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------------------
extern "C" int slq_device_count(int *count) {
  if (!count) return fail(SLQ_EINVAL, "count is NULL");
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) {
    *count = 0;
    return fail(SLQ_ENODEV, "hipGetDeviceCount: %s", hipGetErrorString(e));
  }
  *count = c;
  return SLQ_OK;
}

extern "C" int slq_context_create(int device, void *hip_stream, slq_context **out) {
  if (!out) return fail(SLQ_EINVAL, "out is NULL");
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
    return fail(SLQ_ENODEV, "no HIP device visible: the SLQ engine has no CPU fallback");
  if (device < 0) HIP_TRY(hipGetDevice(&device));
  if (device >= count) return fail(SLQ_EINVAL, "device %d out of range (%d visible)", device, count);
  HIP_TRY(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(SLQ_ENODEV, "device %d is %s; libslq is built for gfx950 only", device,
                prop.gcnArchName);
  slq_context *ctx = new (std::nothrow) slq_context();
  if (!ctx) return fail(SLQ_ENOMEM, "host allocation failed");
  ctx->device = device;
  ctx->num_cus = prop.multiProcessorCount;
  if (hip_stream) {
    ctx->stream = (hipStream_t)hip_stream;
    ctx->own_stream = false;
  } else {
    hipError_t e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
      delete ctx;
      return fail(SLQ_EHIP, "hipStreamCreate: %s", hipGetErrorString(e));
    }
    ctx->own_stream = true;
  }
  *out = ctx;
  return SLQ_OK;
}

extern "C" int slq_context_destroy(slq_context *ctx) {
  if (!ctx) return SLQ_OK;
  ctx->dead = true;
  if (ctx->refs == 0) ctx_free(ctx);
  return SLQ_OK;
}

extern "C" int slq_context_synchronize(slq_context *ctx) {
  if (!ctx) return fail(SLQ_EINVAL, "ctx is NULL");
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return SLQ_OK;
}

extern "C" int slq_context_device(slq_context *ctx, int *device) {
  if (!ctx || !device) return fail(SLQ_EINVAL, "ctx/device is NULL");
  *device = ctx->device;
  return SLQ_OK;
}

extern "C" int slq_context_meminfo(slq_context *ctx, size_t *free_bytes, size_t *total_bytes) {
  if (!ctx) return fail(SLQ_EINVAL, "ctx is NULL");
  HIP_TRY(hipSetDevice(ctx->device));
  size_t f = 0, t = 0;
  HIP_TRY(hipMemGetInfo(&f, &t));
  if (free_bytes) *free_bytes = f;
  if (total_bytes) *total_bytes = t;
  return SLQ_OK;
}

// ---------------------------------------------------------------------------------------------------
// operators
// ---------------------------------------------------------------------------------------------------
static size_t esize(int dtype) { return dtype == SLQ_F64 ? 8 : 4; }

static int check_dtype(int dtype) {
  if (dtype != SLQ_F32 && dtype != SLQ_F64)
    return fail(SLQ_EINVAL, "Only 32- or 64-bit floats are supported.");
  return SLQ_OK;
}


// ---- derived data built on the device (slq_build.hpp) ----
// a[0, count) := its inclusive scan (the callers keep a zero in front of it: row pointers, record offsets)
static hipError_t device_scan_inclusive(int32_t *a, int64_t count, hipStream_t st) {
  if (count <= 0) return hipSuccess;
  const int nb = (int)((count + slqb::kScanTile - 1) / slqb::kScanTile);
  DevBuf sums;
  hipError_t e = sums.alloc((size_t)nb * 4);
  if (e != hipSuccess) return e;
  slqb::k_scan_block_sums<<<dim3(nb), dim3(256), 0, st>>>(a, count, sums.as<int32_t>());
  slqb::k_scan_sums<<<dim3(1), dim3(1024), 0, st>>>(sums.as<int32_t>(), nb);
  slqb::k_scan_apply<<<dim3(nb), dim3(256), 0, st>>>(a, count, sums.as<int32_t>());
  e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(st);  // (sums is freed on return)
  return e;
}
// The descriptor / record stream of R-merged tiles `tile_row_d` (device, ntiles + 1) over the CSR (rp, ci, va) (device): what
// build_tile_meta + build_ring_stream produce on the host, byte for byte. want_pad: rows padded to whole chunks of four entries
// unless some record would outgrow its slot (out.padded tells). max_lines_per_row > 0: nothing is built (return 1) when the tiles
// land more distinct panel rows per row than that; out.max_lines / *sum_lines are set either way. tile_ptr (optional): [ntiles + 1]
// running sum of the lists' lengths. 0: built; < 0: failed (the SLQ status). out.xcd_tile is the caller's to set.
static int device_build_stream(slq_context *ctx, int dtype, int R, int64_t n, const int32_t *rp, const int32_t *ci, const void *va, const int32_t *tile_row_d,
                               int ntiles, bool want_pad, double max_lines_per_row, TileStream &out, int64_t *sum_lines = nullptr, DevBuf *tile_ptr = nullptr) {
  hipStream_t st = ctx->stream;
  const int cap = kRingTileCols * R;
  const int es = (int)esize(dtype);
  const int head_bytes = kRecHeadBytes * R, pad_limit = (kRingRecStride * R + 1023) / 1024 * 1024;
  DevBuf lists, small;
  const size_t cnt = (size_t)ntiles + 1;
  hipError_t e = lists.alloc((size_t)ntiles * cap * 4);
  if (e == hipSuccess) e = small.alloc((3 * cnt + 4) * 4);
  if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? SLQ_ENOMEM : SLQ_EHIP, "tile stream scratch: %s", hipGetErrorString(e));
  int32_t *D = small.as<int32_t>(), *units = D + cnt, *units_pad = units + cnt;
  int *flags = (int *)(units_pad + cnt);
  e = hipMemsetAsync(small.p, 0, (3 * cnt + 4) * 4, st);
  if (e != hipSuccess) return fail(SLQ_EHIP, "tile stream scratch: %s", hipGetErrorString(e));
  const dim3 gl((unsigned)((ntiles + 63) / 64));
  if (R == 1) slqb::k_tile_lists<kRingTileCols><<<gl, dim3(64), 0, st>>>(ntiles, rp, ci, tile_row_d, lists.as<int32_t>(), D, units, units_pad, head_bytes, es, pad_limit, flags);
  else if (R == 2) slqb::k_tile_lists<2 * kRingTileCols><<<gl, dim3(64), 0, st>>>(ntiles, rp, ci, tile_row_d, lists.as<int32_t>(), D, units, units_pad, head_bytes, es, pad_limit, flags);
  else if (R == 4) slqb::k_tile_lists<4 * kRingTileCols><<<gl, dim3(64), 0, st>>>(ntiles, rp, ci, tile_row_d, lists.as<int32_t>(), D, units, units_pad, head_bytes, es, pad_limit, flags);
  else return fail(SLQ_EINVAL, "tiles are merged 1, 2 or 4 at a time");
  int hflags[4] = {0, 0, 0, 0};
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(hflags, flags, sizeof hflags, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return fail(SLQ_EHIP, "tile lists: %s", hipGetErrorString(e));
  if (hflags[0]) return fail(SLQ_EHIP, "a tile lists more than %d distinct panel rows (tiles not built to the ring's caps)", cap);
  out.max_lines = hflags[2];
  out.padded = want_pad && !hflags[1];
  int32_t *u = out.padded ? units_pad : units;
  e = device_scan_inclusive(D + 1, ntiles, st);
  if (e == hipSuccess) e = device_scan_inclusive(u + 1, ntiles, st);
  int32_t totals[2] = {0, 0};
  if (e == hipSuccess) e = hipMemcpyAsync(&totals[0], D + ntiles, 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(&totals[1], u + ntiles, 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return fail(SLQ_EHIP, "tile stream offsets: %s", hipGetErrorString(e));
  if (sum_lines) *sum_lines = totals[0];
  if (max_lines_per_row > 0.0 && (double)totals[0] / (double)n > max_lines_per_row) {
    out.padded = false;
    return 1;
  }
  DevBuf &desc = out.desc, &rec = out.rec;
  e = desc.alloc((size_t)ntiles * 64 * R * 4);
  if (e == hipSuccess) e = rec.alloc((size_t)totals[1] * 16 + (size_t)kRingMetaBytes * R);
  if (e == hipSuccess && tile_ptr) e = tile_ptr->alloc(cnt * 4);
  if (e == hipSuccess && tile_ptr) e = hipMemcpyAsync(tile_ptr->p, D, cnt * 4, hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync(rec.as<char>() + (size_t)totals[1] * 16, 0, (size_t)kRingMetaBytes * R, st);  // the spare record behind the last one
  if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? SLQ_ENOMEM : SLQ_EHIP, "tile stream: %s", hipGetErrorString(e));
  const dim3 gs((unsigned)((ntiles + 3) / 4));
  const int pad = out.padded ? 1 : 0;
#define SLQ_STREAM_LAUNCH(F, CAP) \
  slqb::k_tile_stream<F, CAP><<<gs, dim3(256), 0, st>>>(ntiles, R, pad, rp, ci, (const F *)va, tile_row_d, lists.as<int32_t>(), D, u, desc.as<int32_t>(), rec.as<char>())
  if (dtype == SLQ_F64) {
    if (R == 1) SLQ_STREAM_LAUNCH(double, kRingTileCols);
    else if (R == 2) SLQ_STREAM_LAUNCH(double, 2 * kRingTileCols);
    else SLQ_STREAM_LAUNCH(double, 4 * kRingTileCols);
  } else {
    if (R == 1) SLQ_STREAM_LAUNCH(float, kRingTileCols);
    else if (R == 2) SLQ_STREAM_LAUNCH(float, 2 * kRingTileCols);
    else SLQ_STREAM_LAUNCH(float, 4 * kRingTileCols);
  }
#undef SLQ_STREAM_LAUNCH
  e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(st);  // (the scratch goes when this returns)
  if (e != hipSuccess) return fail(SLQ_EHIP, "tile stream: %s", hipGetErrorString(e));
  return 0;
}
// the same bytes on the device and on the host / twice on the device (null pointers: equal when both are) - what SLQ_DEVICE_BUILD=2 compares
static bool device_equals_host(const void *dev, const void *host, size_t bytes) {
  std::vector<char> tmp(bytes);
  if (hipMemcpy(tmp.data(), dev, bytes, hipMemcpyDeviceToHost) != hipSuccess) return false;
  return memcmp(tmp.data(), host, bytes) == 0;
}
static bool device_equals_device(const void *x, const void *y, size_t bytes) {
  if (!x || !y) return x == y;
  std::vector<char> hx(bytes);
  return hipMemcpy(hx.data(), x, bytes, hipMemcpyDeviceToHost) == hipSuccess && device_equals_host(y, hx.data(), bytes);
}
static bool buffers_equal(const DevBuf &x, const DevBuf &y) { return x.bytes() == y.bytes() && device_equals_device(x.p, y.p, x.bytes()); }
// 0 when two tile streams are the same, else what differs first: 1 one is built and the other is not, or their sizes, tile ranges,
// longest lists or padding; 2 the descriptors; 3 the records
static int streams_differ(const TileStream &a, const TileStream &b) {
  if ((bool)a != (bool)b || a.desc.bytes() != b.desc.bytes() || a.rec.bytes() != b.rec.bytes()) return 1;
  if (!std::equal(a.xcd_tile, a.xcd_tile + 9, b.xcd_tile) || a.max_lines != b.max_lines || a.padded != b.padded) return 1;
  if (!buffers_equal(a.desc, b.desc)) return 2;
  return buffers_equal(a.rec, b.rec) ? 0 : 3;
}

// No C++ exception crosses the C boundary: every slq_*_create whose body allocates on the host runs it through here, and
// holds the operator it is building in an OpGuard - however the body is left without handing the operator out (an error
// return, an exception of the host-side analysis), the operator and what it owns on the device go with it.
template <typename Body> static int create_guarded(slq_operator **out, Body body) {
  try {
    return body();
  } catch (const std::bad_alloc &) {
    if (out) *out = nullptr;
    return fail(SLQ_ENOMEM, "host allocation failed while analysing the operator");
  } catch (const std::exception &e) {  // (e.g. no thread to be had)
    if (out) *out = nullptr;
    return fail(SLQ_EHIP, "operator analysis failed: %s", e.what());
  }
}
// What every slq_*_create begins with: the arguments every kind shares are checked, the context's device is made current, and a new
// operator of `kind` holds the context and the switches as they are now (the one read of a creation). The caller puts it in an OpGuard.
static int operator_new(slq_context *ctx, int kind, int dtype, int64_t n, int64_t nnz, slq_operator **out, slq_operator **op) {
  if (!ctx || !out) return fail(SLQ_EINVAL, "ctx/out is NULL");
  *out = nullptr;
  SLQ_TRY(check_dtype(dtype));
  HIP_TRY(hipSetDevice(ctx->device));
  if (ctx->dead) return fail(SLQ_EINVAL, "the context has been destroyed");
  slq_operator *o = new (std::nothrow) slq_operator();
  if (!o) return fail(SLQ_ENOMEM, "host allocation failed");
  ctx_retain(ctx);
  o->ctx = ctx, o->kind = kind, o->dtype = dtype, o->n = n, o->nnz = nnz;
  o->sw = read_operator_switches();
  *op = o;
  return SLQ_OK;
}
struct OpGuard {  // (declare it BEFORE an upload queue that fills the operator's arrays: that one joins first)
  slq_operator *op;
  ~OpGuard() {
    if (op) slq_operator_destroy(op);
  }
  slq_operator *release() {
    slq_operator *o = op;
    op = nullptr;
    return o;
  }
};
// plain != 0: rows stay in the caller's order and no derived copy (upper triangle, tiles) is built - for operators whose
// values change after creation (the affine operator)
// dev: the same CSR already on the device (slq_csr_create_device): the device-side build reads it in place, and `vals` may then be null
// (the values come back to the host only if the host has to build the operator after all)
struct DeviceCsr { const int32_t *rp = nullptr, *ci = nullptr; const void *va = nullptr; };
static int csr_create_body(slq_context *ctx, int dtype, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colind,
                           const void *vals, slq_operator **out, int plain, int host_build, DeviceCsr dev);
static int csr_create_impl(slq_context *ctx, int dtype, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colind,
                           const void *vals, slq_operator **out, int plain, int host_build = 0, DeviceCsr dev = DeviceCsr()) {
  return create_guarded(out, [&]() { return csr_create_body(ctx, dtype, n, nnz, rowptr, colind, vals, out, plain, host_build, dev); });
}

extern "C" int slq_csr_create(slq_context *ctx, int dtype, int64_t n, int64_t nnz,
                              const int32_t *rowptr, const int32_t *colind, const void *vals,
                              slq_operator **out) {
  return csr_create_impl(ctx, dtype, n, nnz, rowptr, colind, vals, out, 0);
}

// what both storage builders print under SLQ_DEBUG
static void debug_stored_csr(const slq_operator *op, const char *how) {
  if (op->sw.debug != 0)
    fprintf(stderr, "[slq] csr n=%lld nnz=%lld reordered=%d rms in-chunk |i-j| = %.1f, far gathers per row %.2f%s\n", (long long)op->n,
            (long long)op->nnz, op->perm_h.empty() ? 0 : 1, op->rms_dist, op->far_per_row, how);
}
static void debug_upper_tiles(const slq_operator *op, size_t ntu, size_t ntiles) {
  if (op->sw.debug != 0)
    fprintf(stderr, "[slq] tiles: upper-triangle stream on %zu tiles of %.2f rows (base: %zu of %.2f)\n", ntu, (double)op->n / (double)ntu, ntiles,
            (double)op->n / (double)ntiles);
}
static void debug_upper_lists(const slq_operator *op) {
  if (op->sw.debug != 0)
    fprintf(stderr, "[slq] tiles: upper triangle: %.2f distinct panel rows per row, longest list %d (full rows: %d)\n", op->upper_per_row,
            op->streams[0].upper.max_lines, op->tiles.max_cols);
}

// The host side of one tile stream: the tiles' lists (build_tile_meta) and the stream made of them, which an upload reads - so it
// outlives the wait for the queue the upload was pushed into (declare it BEFORE that queue).
struct HostStream {
  std::vector<int32_t> tp, tc, lc, si;
  int max_cols = 0;
  RawBuf<int32_t> desc;
  RawBuf<char> rec;
};
struct HostCsr { const int32_t *rowptr, *colind; const void *vals; };
// The stream of the R-merged tiles `tile_row` over a CSR on the host: lists, descriptors and records (build_tile_meta +
// build_ring_stream), their device arrays in `out`, the upload pushed into `up`; h keeps the lists for whoever needs them. As with
// device_build_stream, out.max_lines is set either way, want_pad asks for padded rows (out.padded tells), out.xcd_tile is the
// caller's to set, and `out` stays empty when the tiles land more than max_lines_per_row (> 0) distinct panel rows per row - or
// when a list outgrows the ring's cap.
static hipError_t host_build_stream(const slq_operator *op, int R, const HostCsr &A, const std::vector<int32_t> &tile_row, bool want_pad, double max_lines_per_row,
                                    HostStream &h, UploadQueue &up, TileStream &out, PhaseClock *clk = nullptr, const char *what = "") {
  build_tile_meta(op->n, A.rowptr, A.colind, tile_row, h.tp, h.tc, h.lc, h.si, &h.max_cols, op->sw);
  if (clk) clk->lap((std::string("  ") + what + "tile lists").c_str());
  out.max_lines = h.max_cols;
  if (h.max_cols > kRingTileCols * R) return hipSuccess;
  if (max_lines_per_row > 0.0 && (double)(h.tc.size() - kCsrPad) / (double)op->n > max_lines_per_row) return hipSuccess;
  bool pad = want_pad;
  if (op->dtype == SLQ_F64) build_ring_stream<double>(R, A.rowptr, (const double *)A.vals, tile_row, h.tp, h.tc, h.lc, h.si, h.desc, h.rec, &pad);
  else build_ring_stream<float>(R, A.rowptr, (const float *)A.vals, tile_row, h.tp, h.tc, h.lc, h.si, h.desc, h.rec, &pad);
  out.padded = pad;
  if (clk) clk->lap((std::string("  ") + what + "tile stream").c_str());
  hipError_t e = out.desc.alloc(h.desc.size() * 4);
  if (e == hipSuccess) e = out.rec.alloc(h.rec.size());
  if (e == hipSuccess) up.push({{out.desc.p, h.desc.data(), h.desc.size() * 4}, {out.rec.p, h.rec.data(), h.rec.size()}});
  return e;
}

// An operator's storage built on the host from its layout: the permuted CSR, the far-gather count, the upper triangle, the tile
// lists and both tile streams. Every array goes to the device through `up` while the next one is being built; the buffers it
// reads are declared before it (L lives in the caller) and nothing returns without up.wait() (its destructor, at the latest).
static int build_storage_host(slq_context *ctx, slq_operator *op, const CsrView &A, const void *vals, const OperatorLayout &L, int plain, PhaseClock &clk) {
  const int64_t n = A.n, nnz = A.nnz;
  const int32_t *rowptr = A.rowptr, *colind = A.colind;
  const int dtype = op->dtype;
  const size_t es = esize(dtype);
  const OperatorSwitches &osw = op->sw;
  const std::vector<int32_t> &tile_row = L.tile_row;
  RawBuf<int32_t> ci2;                            // the stored CSR of a reordered operator: A' = P A P^T, vectors live in the permuted row space
  RawBuf<char> va2;
  std::vector<int32_t> urp, uci;                  // the upper triangle (stored order), also the source of the alpha-only tile stream
  std::vector<char> uva;
  HostStream hs, hsu;  // (the upper stream in buffers of its own: the full stream's upload is still running when it is built)
  UploadQueue up(ctx->device);
  auto bail = [&](int code, const char *what, hipError_t e) {
    up.wait();
    hipStreamSynchronize(ctx->stream);
    return fail(e == hipErrorOutOfMemory ? SLQ_ENOMEM : code, "%s: %s", what, hipGetErrorString(e));
  };
  if (!op->perm_h.empty()) {
    const std::vector<int32_t> &perm = op->perm_h, &inv = L.inv, &rp2 = L.rowptr_stored;
    hipError_t pe = op->perm_d.alloc((size_t)n * 4);
    if (pe == hipSuccess) pe = op->inv_perm_d.alloc((size_t)n * 4);
    if (pe != hipSuccess) return bail(SLQ_EHIP, "permutation upload", pe);
    up.push({{op->perm_d.p, perm.data(), (size_t)n * 4}, {op->inv_perm_d.p, inv.data(), (size_t)n * 4}});
    ci2.alloc((size_t)nnz);
    va2.alloc((size_t)nnz * es);
    const bool pok = parallel_pieces(host_threads(), n, [&](int, int64_t i0, int64_t i1) {
      std::vector<std::pair<int32_t, int32_t>> rowbuf;
      for (int64_t i = i0; i < i1; ++i) {
        const int32_t o = perm[(size_t)i];
        rowbuf.clear();
        for (int32_t q = rowptr[o]; q < rowptr[o + 1]; ++q) rowbuf.emplace_back(inv[(size_t)colind[q]], q);
        std::sort(rowbuf.begin(), rowbuf.end());
        int32_t w = rp2[(size_t)i];
        for (auto &e2 : rowbuf) {
          ci2.data()[(size_t)w] = e2.first;
          memcpy(va2.data() + (size_t)w * es, (const char *)vals + (size_t)e2.second * es, es);
          ++w;
        }
      }
    });
    if (!pok) {
      return fail(SLQ_ENOMEM, "host allocation failed");
    }
    rowptr = rp2.data();
    colind = ci2.data();
    vals = va2.data();
  }
  clk.lap("permuted CSR");
  hipError_t e = op->csr.alloc(n, nnz, es, ctx->stream);
  if (e != hipSuccess) return bail(SLQ_EHIP, "CSR upload", e);
  up.push({{op->csr.rowptr.p, rowptr, (size_t)(n + 1) * 4}, {op->csr.colind.p, colind, (size_t)nnz * 4}, {op->csr.vals.p, vals, (size_t)nnz * es}});
  {
    // gathers per row that reach further than any cache-resident halo (|i - j| > 4096 rows in the stored
    // order): what decides between the recompute passes and the store-and-revisit sweeps (enqueue_run)
    std::vector<int64_t> farp((size_t)host_threads(), 0);
    if (!parallel_pieces((int)farp.size(), n, [&](int piece, int64_t i0, int64_t i1) {
      int64_t f = 0;
      for (int64_t i = i0; i < i1; ++i)
        for (int32_t q = rowptr[i]; q < rowptr[i + 1]; ++q) f += std::llabs((long long)colind[q] - (long long)i) > 4096;
      farp[(size_t)piece] = f;
    })) return bail(SLQ_ENOMEM, "host worker failed (far-gather count)", hipSuccess);
    int64_t far = 0;
    for (int64_t f : farp) far += f;
    op->far_per_row = (double)far / (double)n;
  }
  debug_stored_csr(op, "");
  clk.lap("far count");
  // Symmetric operators (what Lanczos assumes; the reference never checks): the alpha pass only needs the
  // scalar q^T A q, so it can run on the upper triangle with doubled off-diagonals and gather half the
  // panel rows. Built only when the stored CSR is EXACTLY symmetric (pattern and values, sorted rows
  // without duplicates); anything else keeps the full rows. SLQ_SYM_ALPHA=0 disables it.
  bool sym = false;
  if (!plain && osw.sym_alpha != 0 && nnz > 0) {
    sym = dtype == SLQ_F64 ? build_symmetric_upper<double>(n, rowptr, colind, (const double *)vals, urp, uci, uva)
                                : build_symmetric_upper<float>(n, rowptr, colind, (const float *)vals, urp, uci, uva);
    if (sym) {
      const size_t nu = uci.size();
      const hipError_t ue = op->upper.alloc(n, (int64_t)nu, es, ctx->stream);
      if (ue != hipSuccess) return bail(SLQ_EHIP, "upper-triangle upload", ue);
      up.push({{op->upper.rowptr.p, urp.data(), (size_t)(n + 1) * 4}, {op->upper.colind.p, uci.data(), nu * 4}, {op->upper.vals.p, uva.data(), nu * es}});
    }
  }
  clk.lap("upper triangle");
  // workgroup tiles (SLQ_TILES): lists of the stored CSR, uploaded next to it
  if (L.have_tiles) {
    slq_operator::TileLists &T = op->tiles;
    TileStreamPair &base = op->streams[0];
    op->tiles_ringed = osw.tiles == 2;
    hipError_t te = hipSuccess;
    if (op->tiles_ringed) {
      te = host_build_stream(op, 1, HostCsr{rowptr, colind, vals}, tile_row, false, 0.0, hs, up, base.full, &clk);
    } else {
      build_tile_meta(n, rowptr, colind, tile_row, hs.tp, hs.tc, hs.lc, hs.si, &hs.max_cols, osw);
      clk.lap("  tile lists");
    }
    if (te == hipSuccess) te = T.tile_row.alloc(tile_row.size() * 4);
    if (te == hipSuccess) te = T.tile_ptr.alloc(hs.tp.size() * 4);
    if (te == hipSuccess) up.push({{T.tile_row.p, tile_row.data(), tile_row.size() * 4}, {T.tile_ptr.p, hs.tp.data(), hs.tp.size() * 4}});
    // (the per-nonzero lists are read by k_csr_tile_pass only: ring-sized tiles carry them inside their records instead)
    if (te == hipSuccess && !op->tiles_ringed) te = T.tile_cols.alloc(hs.tc.size() * 4);
    if (te == hipSuccess && !op->tiles_ringed) te = T.lcol.alloc(hs.lc.size() * 4);
    if (te == hipSuccess && !op->tiles_ringed) te = T.self_idx.alloc(hs.si.size() * 4);
    if (te == hipSuccess && !op->tiles_ringed)
      up.push({{T.tile_cols.p, hs.tc.data(), hs.tc.size() * 4}, {T.lcol.p, hs.lc.data(), hs.lc.size() * 4}, {T.self_idx.p, hs.si.data(), hs.si.size() * 4}});
    std::copy(L.xcd_tile, L.xcd_tile + 9, T.xcd_tile);
    std::copy(L.xcd_tile, L.xcd_tile + 9, base.full.xcd_tile);
    T.max_cols = hs.max_cols;
    if (te == hipSuccess && op->tiles_ringed && sym) {
      // the same tiles over the upper triangle (doubled off-diagonals), for the alpha-only pass: a tile's image then holds its
      // own rows and the neighbours of HIGHER index only - about half the halo, and the pass is bound by what it lands by DMA
      // (its own, longer tiles: runs of the base tiles - the pass pays per tile, regroup_upper_tiles; SLQ_RING_UPPER_REGROUP=0 keeps the base tiles)
      std::vector<int32_t> tile_row_u;
      if (regroup_upper_wanted(osw, n, tile_row.size() - 1)) {
        regroup_upper_tiles(urp.data(), uci.data(), tile_row, L.xcd_tile, tile_row_u, base.upper.xcd_tile);
      } else {
        tile_row_u = tile_row;
        std::copy(L.xcd_tile, L.xcd_tile + 9, base.upper.xcd_tile);
      }
      debug_upper_tiles(op, tile_row_u.size() - 1, tile_row.size() - 1);
      // Worth it while the tiles land at most kTileAlphaColsPerRow panel rows per row (r03, scalar-descriptor loaders and the
      // padded-row consumer of slq_ring.hpp: 5-point grid, 1.5 rows per row: 0.40 against 0.51 ms for the generic pass; 7-point
      // grid, 2.5: 0.66 against 0.81 ms)
      // (built up to kTileAlphaMergedColsPerRow: wide panels take it up to kTileAlphaColsPerRow, slq_plan_create; the merged
      // tiles of narrow panels share more of their halo and gain from it on 7-point grids too - 100^3, 64 probes: alpha pass
      // 0.25 against 0.35 ms for the generic upper-triangle pass)
      te = host_build_stream(op, 1, HostCsr{urp.data(), uci.data(), uva.data()}, tile_row_u, osw.ring_pad_rows != 0, kTileAlphaMergedColsPerRow, hsu, up, base.upper,
                             &clk, "upper ");
      op->upper_per_row = (double)(hsu.tc.size() - kCsrPad) / (double)n;
      debug_upper_lists(op);
    }
    if (te != hipSuccess) return bail(SLQ_EHIP, "tile upload", te);
  }
  e = up.wait();
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return bail(SLQ_EHIP, "operator upload", e);
  clk.lap("uploads drained");
  return SLQ_OK;
}

// The same storage for operators with ring-sized tiles, built on the device (SLQ_DEVICE_BUILD, slq_build.hpp) from the caller's CSR
// (src: on its way up through `early`, or the caller's own device arrays): the permuted CSR, the far-gather count, the symmetry check and
// the upper triangle, both tile streams. The one sequential piece left - the runs of base tiles the upper-triangle stream's tiles are
// made of (regroup_upper_tiles_permuted) - runs on a host thread meanwhile, on the caller's CSR seen through the permutation.
static int build_storage_device(slq_context *ctx, slq_operator *op, const CsrView &A, const DeviceCsr &src, UploadQueue &early, const OperatorLayout &L, PhaseClock &clk) {
  hipStream_t st = ctx->stream;
  const int64_t n = A.n, nnz = A.nnz;
  const int dtype = op->dtype;
  const size_t es = esize(dtype);
  const std::vector<int32_t> &perm = op->perm_h, &tile_row = L.tile_row;
  const int ntiles = (int)tile_row.size() - 1;
  const OperatorSwitches &osw = op->sw;
  const bool want_sym = osw.sym_alpha != 0;
  const bool regroup = want_sym && regroup_upper_wanted(osw, n, (size_t)ntiles);
  std::vector<int32_t> tile_row_u;
  int32_t xcd_u[9];
  for (int x = 0; x < 9; ++x) xcd_u[x] = L.xcd_tile[x];
  std::atomic<int> rg_failed{0};
  auto do_regroup = [&]() {
    try {
      regroup_upper_tiles_permuted(A.rowptr, A.colind, perm, L.inv, tile_row, L.xcd_tile, tile_row_u, xcd_u);
    } catch (...) {
      rg_failed = 1;
    }
  };
  std::thread rg;
  struct Joiner {
    std::thread &t;
    ~Joiner() {
      if (t.joinable()) t.join();
    }
  } joiner{rg};
  if (regroup) {
    try {
      rg = std::thread(do_regroup);
    } catch (const std::system_error &) {
      do_regroup();
    }
  }
  auto hip_fail = [&](const char *what, hipError_t e) { return fail(e == hipErrorOutOfMemory ? SLQ_ENOMEM : SLQ_EHIP, "%s: %s", what, hipGetErrorString(e)); };
  CsrArrays &S = op->csr, &U = op->upper;
  DevBuf &d_tr = op->tiles.tile_row;
  hipError_t e = op->perm_d.alloc((size_t)n * 4);
  if (e == hipSuccess) e = op->inv_perm_d.alloc((size_t)n * 4);
  if (e == hipSuccess) e = S.alloc(n, nnz, es, st);
  if (e == hipSuccess) e = d_tr.alloc(tile_row.size() * 4);
  if (e == hipSuccess) e = hipMemcpy(op->perm_d.p, perm.data(), (size_t)n * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(op->inv_perm_d.p, L.inv.data(), (size_t)n * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(S.rowptr.p, L.rowptr_stored.data(), (size_t)(n + 1) * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_tr.p, tile_row.data(), tile_row.size() * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = early.wait();
  if (e != hipSuccess) return hip_fail("CSR upload", e);
  clk.lap("  order, tile boundaries and the caller's CSR on the device");
  const dim3 grow((unsigned)((n + 255) / 256)), brow(256);
  if (dtype == SLQ_F64) slqb::k_permute_csr<double><<<grow, brow, 0, st>>>((int)n, src.rp, src.ci, (const double *)src.va, op->perm_d.as<int32_t>(), op->inv_perm_d.as<int32_t>(), S.rp(), S.colind.as<int32_t>(), S.vals.as<double>());
  else slqb::k_permute_csr<float><<<grow, brow, 0, st>>>((int)n, src.rp, src.ci, (const float *)src.va, op->perm_d.as<int32_t>(), op->inv_perm_d.as<int32_t>(), S.rp(), S.colind.as<int32_t>(), S.vals.as<float>());
  DevBuf misc;  // [0..1] far gathers (u64), [2] "not symmetric"
  e = misc.alloc(16);
  if (e == hipSuccess) e = hipMemsetAsync(misc.p, 0, 16, st);
  if (e != hipSuccess) return hip_fail("operator analysis", e);
  slqb::k_far_count<<<grow, brow, 0, st>>>((int)n, S.rp(), S.ci(), misc.as<unsigned long long>());
  if (want_sym) {
    e = U.rowptr.alloc((size_t)(n + 1) * 4);
    if (e == hipSuccess) e = hipMemsetAsync(U.rowptr.p, 0, 4, st);
    if (e != hipSuccess) return hip_fail("upper triangle", e);
    if (dtype == SLQ_F64) slqb::k_sym_count<double><<<grow, brow, 0, st>>>((int)n, S.rp(), S.ci(), S.vals.as<double>(), U.rowptr.as<int32_t>(), misc.as<int>() + 2);
    else slqb::k_sym_count<float><<<grow, brow, 0, st>>>((int)n, S.rp(), S.ci(), S.vals.as<float>(), U.rowptr.as<int32_t>(), misc.as<int>() + 2);
  }
  struct { unsigned long long far; int bad, spare; } h = {0, 0, 0};
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(&h, misc.p, 16, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return hip_fail("operator analysis", e);
  op->far_per_row = (double)h.far / (double)n;
  bool sym = want_sym && !h.bad;
  if (!sym) U.release();
  if (sym) {
    e = device_scan_inclusive(U.rowptr.as<int32_t>() + 1, n, st);
    int32_t nu32 = 0;
    if (e == hipSuccess) e = hipMemcpy(&nu32, U.rowptr.as<int32_t>() + n, 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = U.alloc_entries((int64_t)nu32, es, st);
    if (e != hipSuccess) return hip_fail("upper triangle", e);
    if (dtype == SLQ_F64) slqb::k_upper_fill<double><<<grow, brow, 0, st>>>((int)n, S.rp(), S.ci(), S.vals.as<double>(), U.rp(), U.colind.as<int32_t>(), U.vals.as<double>());
    else slqb::k_upper_fill<float><<<grow, brow, 0, st>>>((int)n, S.rp(), S.ci(), S.vals.as<float>(), U.rp(), U.colind.as<int32_t>(), U.vals.as<float>());
  }
  debug_stored_csr(op, " (built on the device)");
  clk.lap("  device: stored CSR, upper triangle");
  // the tiles' stream over the full rows
  TileStreamPair &base = op->streams[0];
  int rc = device_build_stream(ctx, dtype, 1, n, S.rp(), S.ci(), S.vals.p, d_tr.as<int32_t>(), ntiles, false, 0.0, base.full, nullptr, &op->tiles.tile_ptr);
  if (rc != 0) return rc < 0 ? rc : fail(SLQ_EHIP, "tile stream declined");
  op->tiles.max_cols = base.full.max_lines;
  std::copy(L.xcd_tile, L.xcd_tile + 9, op->tiles.xcd_tile);
  std::copy(L.xcd_tile, L.xcd_tile + 9, base.full.xcd_tile);
  op->tiles_ringed = true;
  clk.lap("  device: tile stream");
  if (sym) {
    if (rg.joinable()) rg.join();
    if (rg_failed) return fail(SLQ_ENOMEM, "host worker failed (upper-triangle tiles)");
    if (!regroup) tile_row_u = tile_row;
    std::copy(xcd_u, xcd_u + 9, base.upper.xcd_tile);
    const int ntu = (int)tile_row_u.size() - 1;
    debug_upper_tiles(op, (size_t)ntu, (size_t)ntiles);
    DevBuf d_tru;
    e = d_tru.alloc(tile_row_u.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(d_tru.p, tile_row_u.data(), tile_row_u.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail("upper-triangle tiles", e);
    int64_t sum_lines = 0;
    rc = device_build_stream(ctx, dtype, 1, n, U.rp(), U.ci(), U.vals.p, d_tru.as<int32_t>(), ntu, osw.ring_pad_rows != 0, kTileAlphaMergedColsPerRow, base.upper, &sum_lines);
    if (rc < 0) return rc;
    op->upper_per_row = (double)sum_lines / (double)n;
    debug_upper_lists(op);
    clk.lap("  device: upper tile stream");
  }
  e = hipStreamSynchronize(st);
  if (e != hipSuccess) return hip_fail("operator build", e);
  return SLQ_OK;
}

// a square CSR pattern the library can store: int32 shape, row pointer from 0 to nnz and non-decreasing, every column inside [0, n)
static int validate_csr(int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colind) {
  if (n <= 0 || n >= (int64_t)1 << 31 || nnz < 0 || nnz >= (int64_t)1 << 31)
    return fail(SLQ_EINVAL, "CSR shape out of range for int32 indices (n=%lld, nnz=%lld)",
                (long long)n, (long long)nnz);
  if (!rowptr || (nnz > 0 && !colind)) return fail(SLQ_EINVAL, "CSR arrays are NULL");
  if (rowptr[0] != 0 || rowptr[n] != nnz)
    return fail(SLQ_EINVAL, "rowptr[0] must be 0 and rowptr[n] must equal nnz");
  for (int64_t i = 0; i < n; ++i)
    if (rowptr[i + 1] < rowptr[i]) return fail(SLQ_EINVAL, "rowptr is not non-decreasing at %lld", (long long)i);
  // every column index inside [0, n): ranges of the array in parallel, the first offender (lowest position) reported
  const int pieces = host_threads();
  std::vector<int64_t> bad((size_t)pieces, -1);
  if (!parallel_pieces(pieces, nnz, [&](int piece, int64_t p0, int64_t p1) {
        for (int64_t p = p0; p < p1; ++p)
          if (colind[p] < 0 || colind[p] >= n) { bad[(size_t)piece] = p; break; }
      }))
    return fail(SLQ_ENOMEM, "host worker failed while validating the column indices");
  for (int64_t b : bad)
    if (b >= 0) return fail(SLQ_EINVAL, "column index %d out of range at position %lld", colind[b], (long long)b);
  return SLQ_OK;
}

static int operators_differ(const slq_operator *a, const slq_operator *b);
// A CSR operator's creation, phase by phase: validate, layout_prefilter, start the early upload, decide_layout (slq_layout.hpp),
// then one of the two storage builders, which consume the same OperatorLayout.
static int csr_create_body(slq_context *ctx, int dtype, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colind,
                           const void *vals, slq_operator **out, int plain, int host_build, DeviceCsr dev) {
  slq_operator *op = nullptr;
  SLQ_TRY(operator_new(ctx, OP_CSR, dtype, n, nnz, out, &op));
  OpGuard guard{op};
  const OperatorSwitches osw = op->sw;  // (everything below keeps the values the operator was created under; a copy: the analysis reads it in its inner loops)
  PhaseClock clk(osw);
  SLQ_TRY(validate_csr(n, nnz, rowptr, colind));
  if (nnz > 0 && !vals && !dev.va) return fail(SLQ_EINVAL, "CSR arrays are NULL");
  clk.lap("validation");
  const CsrView A{n, nnz, rowptr, colind};
  const LayoutPrefilter pre = layout_prefilter(A, osw, plain != 0);
  clk.lap("tile sample");
  // SLQ_DEVICE_BUILD (r04, slq_build.hpp): 1 (default) - an operator that gets ring-sized tiles has its stored CSR, upper triangle and
  // tile streams built on the device from the caller's CSR, which starts its way up now, while the host orders and clusters the rows;
  // 0 - everything on the host, as before; 2 - both, compared array by array (tests)
  const int dev_mode = (plain || host_build) ? 0 : osw.device_build;
  const bool early_started = dev_mode != 0 && pre.try_tiles && pre.tmode == 2 && pre.reorder_mode != 0 && osw.ring_order == 0;
  DevBuf o_rp, o_ci, o_va;         // the caller's CSR on the device (scratch of the build)
  UploadQueue early(ctx->device);  // (declared after what it fills: joined first)
  DeviceCsr src = dev;             // where the device-side build reads the caller's CSR: in place (slq_csr_create_device), or
  if (early_started && !dev.va) {  // ... from the scratch the early upload fills
    hipError_t ee = o_rp.alloc((size_t)(n + 1) * 4);
    if (ee == hipSuccess) ee = o_ci.alloc((size_t)nnz * 4);
    if (ee == hipSuccess) ee = o_va.alloc((size_t)nnz * esize(dtype));
    if (ee != hipSuccess) return fail(ee == hipErrorOutOfMemory ? SLQ_ENOMEM : SLQ_EHIP, "CSR upload: %s", hipGetErrorString(ee));
    early.push({{o_rp.p, rowptr, (size_t)(n + 1) * 4}, {o_ci.p, colind, (size_t)nnz * 4}, {o_va.p, vals, (size_t)nnz * esize(dtype)}});
    src.rp = o_rp.as<int32_t>(), src.ci = o_ci.as<int32_t>(), src.va = o_va.p;
  }
  OperatorLayout L = decide_layout(A, osw, pre, &clk);
  op->rms_dist = L.rms_dist;
  op->perm_h = std::move(L.perm);  // (the operator keeps the order; the builders read it there)
  std::vector<char> vals_back;  // the values of a device-resident CSR, fetched when the host needs them
  auto need_host_vals = [&]() -> hipError_t {
    if (vals || nnz == 0) return hipSuccess;
    vals_back.resize((size_t)nnz * esize(dtype));
    const hipError_t he = hipMemcpy(vals_back.data(), dev.va, vals_back.size(), hipMemcpyDeviceToHost);
    vals = vals_back.data();
    return he;
  };
  if (early_started && L.have_tiles) {
    SLQ_TRY(build_storage_device(ctx, op, A, src, early, L, clk));
    if (dev_mode == 2) {  // the same operator built on the host: every array must be the same
      if (need_host_vals() != hipSuccess) return fail(SLQ_EHIP, "CSR values: copy back failed");
      slq_operator *ref = nullptr;
      SLQ_TRY(csr_create_impl(ctx, dtype, n, nnz, rowptr, colind, vals, &ref, plain, 1));
      const int diff = operators_differ(op, ref);
      slq_operator_destroy(ref);
      if (diff) return fail(SLQ_EHIP, "the device-built operator differs from the host-built one (SLQ_DEVICE_BUILD=2, item %d)", diff);
    }
  } else {
    if (early_started) {  // no tiles after all: the host builder uploads what it builds
      early.wait();
      o_rp.release(), o_ci.release(), o_va.release();
    }
    if (need_host_vals() != hipSuccess) return fail(SLQ_EHIP, "CSR values: copy back failed");
    SLQ_TRY(build_storage_host(ctx, op, A, vals, L, plain, clk));
  }
  clk.total("all of slq_csr_create");
  *out = guard.release();
  return SLQ_OK;
}

// SLQ_DEVICE_BUILD=2: 0 when everything two operators over the same matrix keep is the same, else the number of the first item that is not
static int operators_differ(const slq_operator *a, const slq_operator *b) {
  auto csr_differ = [](const CsrArrays &x, const CsrArrays &y) {  // 0, or 1 + the array that differs
    if ((bool)x != (bool)y || x.nnz != y.nnz) return 1;
    return !buffers_equal(x.rowptr, y.rowptr) ? 2 : !buffers_equal(x.colind, y.colind) ? 3 : !buffers_equal(x.vals, y.vals) ? 4 : 0;
  };
  if (a->n != b->n || a->nnz != b->nnz || a->dtype != b->dtype) return 1;
  if (a->perm_h.empty() || a->perm_h != b->perm_h) return 2;
  if (!buffers_equal(a->perm_d, b->perm_d) || !buffers_equal(a->inv_perm_d, b->inv_perm_d)) return 3;
  if (int d = csr_differ(a->csr, b->csr)) return 3 + d;  // 4 .. 7
  if (a->far_per_row != b->far_per_row || a->rms_dist != b->rms_dist) return 8;
  if (int d = csr_differ(a->upper, b->upper)) return 8 + d;  // 9 .. 12
  if (!std::equal(a->tiles.xcd_tile, a->tiles.xcd_tile + 9, b->tiles.xcd_tile)) return 13;
  if (!buffers_equal(a->tiles.tile_row, b->tiles.tile_row) || !buffers_equal(a->tiles.tile_ptr, b->tiles.tile_ptr)) return 14;
  if (a->tiles.max_cols != b->tiles.max_cols || a->tiles_ringed != b->tiles_ringed) return 15;
  if (int d = streams_differ(a->streams[0].full, b->streams[0].full)) return 15 + d;  // 16 .. 18
  if (a->upper_per_row != b->upper_per_row) return 19;
  if (int d = streams_differ(a->streams[0].upper, b->streams[0].upper)) return 19 + d;  // 20 .. 22
  return 0;
}

static int csr_create_device_body(slq_context *ctx, int dtype, int64_t n, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_colind,
                                  const void *d_vals, slq_operator **out) {
  if (!ctx || !out) return fail(SLQ_EINVAL, "ctx/out is NULL");
  *out = nullptr;
  SLQ_TRY(check_dtype(dtype));
  if (n <= 0 || n >= (int64_t)1 << 31 || nnz < 0 || nnz >= (int64_t)1 << 31)
    return fail(SLQ_EINVAL, "CSR shape out of range for int32 indices");
  if (!d_rowptr || (nnz > 0 && (!d_colind || !d_vals))) return fail(SLQ_EINVAL, "CSR arrays are NULL");
  HIP_TRY(hipSetDevice(ctx->device));
  if (ctx->dead) return fail(SLQ_EINVAL, "the context has been destroyed");
  // The operator is built the way slq_csr_create builds it - validated, reordered, with its upper triangle and its tiles. Order and
  // tiles are decided on the host, from the index arrays (4 bytes per nonzero come back, once); what the operator stores is then built
  // on the device straight from the caller's arrays (slq_build.hpp) - the values come back only for operators without ring tiles, whose
  // storage the host builds. The caller's arrays are not referenced after the call.
  std::vector<int32_t> rp((size_t)n + 1), ci((size_t)nnz);
  HIP_TRY(hipMemcpy(rp.data(), d_rowptr, ((size_t)n + 1) * 4, hipMemcpyDeviceToHost));
  if (nnz) HIP_TRY(hipMemcpy(ci.data(), d_colind, (size_t)nnz * 4, hipMemcpyDeviceToHost));
  DeviceCsr dev;
  dev.rp = d_rowptr, dev.ci = d_colind, dev.va = d_vals;
  return csr_create_impl(ctx, dtype, n, nnz, rp.data(), ci.data(), nullptr, out, 0, 0, dev);
}
extern "C" int slq_csr_create_device(slq_context *ctx, int dtype, int64_t n, int64_t nnz,
                                     const int32_t *d_rowptr, const int32_t *d_colind,
                                     const void *d_vals, slq_operator **out) {
  return create_guarded(out, [&]() { return csr_create_device_body(ctx, dtype, n, nnz, d_rowptr, d_colind, d_vals, out); });
}

static int csr_gram_create_body(slq_context *ctx, int dtype, int64_t mrows, int64_t ncols, int64_t nnz, const int32_t *rowptr,
                                const int32_t *colind, const void *vals, slq_operator **out) {
  slq_operator *op = nullptr;
  SLQ_TRY(operator_new(ctx, OP_GRAM, dtype, ncols, nnz, out, &op));
  OpGuard guard{op};
  op->mrows = mrows;
  if (mrows <= 0 || ncols <= 0 || mrows >= (int64_t)1 << 31 || ncols >= (int64_t)1 << 31 || nnz < 0 || nnz >= (int64_t)1 << 31)
    return fail(SLQ_EINVAL, "CSR shape out of range for int32 indices");
  if (!rowptr || (nnz > 0 && (!colind || !vals))) return fail(SLQ_EINVAL, "CSR arrays are NULL");
  if (rowptr[0] != 0 || rowptr[mrows] != nnz) return fail(SLQ_EINVAL, "rowptr[0] must be 0 and rowptr[mrows] must equal nnz");
  for (int64_t i = 0; i < mrows; ++i)
    if (rowptr[i + 1] < rowptr[i]) return fail(SLQ_EINVAL, "rowptr is not non-decreasing at %lld", (long long)i);
  for (int64_t q = 0; q < nnz; ++q)
    if (colind[q] < 0 || colind[q] >= ncols) return fail(SLQ_EINVAL, "column index %d out of range at position %lld", colind[q], (long long)q);
  const size_t es = esize(dtype);
  // transpose on the host (counting sort by column; rows of A^T come out with ascending indices)
  std::vector<int32_t> tp((size_t)ncols + 1, 0), tc((size_t)nnz);
  std::vector<char> tv((size_t)nnz * es);
  for (int64_t q = 0; q < nnz; ++q) ++tp[(size_t)colind[q] + 1];
  for (int64_t c = 0; c < ncols; ++c) tp[(size_t)c + 1] += tp[(size_t)c];
  {
    std::vector<int32_t> cur(tp.begin(), tp.end() - 1);
    for (int64_t i = 0; i < mrows; ++i)
      for (int32_t q = rowptr[i]; q < rowptr[i + 1]; ++q) {
        const int32_t w = cur[(size_t)colind[q]]++;
        tc[(size_t)w] = (int32_t)i;
        memcpy(tv.data() + (size_t)w * es, (const char *)vals + (size_t)q * es, es);
      }
  }
  CsrArrays &S = op->csr, &T = op->transposed;
  hipError_t e = S.alloc(mrows, nnz, es, ctx->stream);
  if (e == hipSuccess) e = T.alloc(ncols, nnz, es, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(S.rowptr.p, rowptr, (size_t)(mrows + 1) * 4, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess && nnz) e = hipMemcpyAsync(S.colind.p, colind, (size_t)nnz * 4, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess && nnz) e = hipMemcpyAsync(S.vals.p, vals, (size_t)nnz * es, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(T.rowptr.p, tp.data(), (size_t)(ncols + 1) * 4, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess && nnz) e = hipMemcpyAsync(T.colind.p, tc.data(), (size_t)nnz * 4, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess && nnz) e = hipMemcpyAsync(T.vals.p, tv.data(), (size_t)nnz * es, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? SLQ_ENOMEM : SLQ_EHIP, "Gram operator upload: %s", hipGetErrorString(e));
  *out = guard.release();
  return SLQ_OK;
}
extern "C" int slq_csr_gram_create(slq_context *ctx, int dtype, int64_t mrows, int64_t ncols, int64_t nnz, const int32_t *rowptr,
                                   const int32_t *colind, const void *vals, slq_operator **out) {
  return create_guarded(out, [&]() { return csr_gram_create_body(ctx, dtype, mrows, ncols, nnz, rowptr, colind, vals, out); });
}

// Affine sparse operator A + t B (eigen_operators.h:106-137, SparseEigenAffineOperator): both n x n CSR. The operator is an
// ordinary CSR operator on the UNION pattern - every fused pass applies - whose values are va + t vb, recomputed on the
// device by slq_operator_set_parameter (t = 0 at creation, like the reference's _param).
static int csr_affine_create_body(slq_context *ctx, int dtype, int64_t n, int64_t nnz_a, const int32_t *rp_a, const int32_t *ci_a,
                                  const void *va, int64_t nnz_b, const int32_t *rp_b, const int32_t *ci_b, const void *vb,
                                  slq_operator **out) {
  if (!ctx || !out) return fail(SLQ_EINVAL, "ctx/out is NULL");
  *out = nullptr;
  SLQ_TRY(check_dtype(dtype));
  if (n <= 0 || n >= (int64_t)1 << 31 || nnz_a < 0 || nnz_b < 0 || nnz_a >= (int64_t)1 << 31 || nnz_b >= (int64_t)1 << 31)
    return fail(SLQ_EINVAL, "CSR shape out of range for int32 indices");
  if (!rp_a || !rp_b || (nnz_a > 0 && (!ci_a || !va)) || (nnz_b > 0 && (!ci_b || !vb))) return fail(SLQ_EINVAL, "CSR arrays are NULL");
  if (rp_a[0] != 0 || rp_b[0] != 0 || rp_a[n] != nnz_a || rp_b[n] != nnz_b)
    return fail(SLQ_EINVAL, "rowptr[0] must be 0 and rowptr[n] must equal nnz");
  for (int64_t i = 0; i < n; ++i)
    if (rp_a[i + 1] < rp_a[i] || rp_b[i + 1] < rp_b[i]) return fail(SLQ_EINVAL, "rowptr is not non-decreasing at %lld", (long long)i);
  const size_t es = esize(dtype);
  std::vector<int32_t> rp, ci;
  std::vector<char> ua, ub;
  std::vector<std::pair<int32_t, int>> a_row, b_row;
  const char zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  rp.assign((size_t)n + 1, 0);
  ci.reserve((size_t)std::max(nnz_a, nnz_b));
  for (int64_t i = 0; i < n; ++i) {
    a_row.clear();
    b_row.clear();
    for (int32_t q = rp_a[i]; q < rp_a[i + 1]; ++q) a_row.emplace_back(ci_a[q], q);
    for (int32_t q = rp_b[i]; q < rp_b[i + 1]; ++q) b_row.emplace_back(ci_b[q], q);
    std::sort(a_row.begin(), a_row.end());
    std::sort(b_row.begin(), b_row.end());
    size_t x = 0, y = 0;
    while (x < a_row.size() || y < b_row.size()) {
      const int32_t ca = x < a_row.size() ? a_row[x].first : INT32_MAX, cb = y < b_row.size() ? b_row[y].first : INT32_MAX;
      const int32_t c = std::min(ca, cb);
      if (c < 0 || c >= n) return fail(SLQ_EINVAL, "column index out of range in the affine operator");
      ci.push_back(c);
      ua.insert(ua.end(), zero, zero + es);
      ub.insert(ub.end(), zero, zero + es);
      if (ca == c) { memcpy(ua.data() + ua.size() - es, (const char *)va + (size_t)a_row[x].second * es, es); ++x; }
      if (cb == c) { memcpy(ub.data() + ub.size() - es, (const char *)vb + (size_t)b_row[y].second * es, es); ++y; }
    }
    if (ci.size() >= ((size_t)1 << 31)) return fail(SLQ_EINVAL, "the union pattern exceeds int32 indices");
    rp[(size_t)i + 1] = (int32_t)ci.size();
  }
  const int64_t nnz = (int64_t)ci.size();
  // the union pattern with A's values is an ordinary CSR operator; keep its rows as given (no reordering, no upper-triangle
  // alpha pass: both would have to follow every parameter change)
  slq_operator *op = nullptr;
  const int rc = csr_create_impl(ctx, dtype, n, nnz, rp.data(), ci.data(), ua.data(), &op, 1);
  if (rc != SLQ_OK) return rc;
  OpGuard guard{op};
  hipError_t e = op->vals_a.alloc((size_t)nnz * es);
  if (e == hipSuccess) e = op->vals_b.alloc((size_t)nnz * es);
  if (e == hipSuccess && nnz) e = hipMemcpyAsync(op->vals_a.p, ua.data(), (size_t)nnz * es, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess && nnz) e = hipMemcpyAsync(op->vals_b.p, ub.data(), (size_t)nnz * es, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? SLQ_ENOMEM : SLQ_EHIP, "affine operator upload: %s", hipGetErrorString(e));
  *out = guard.release();
  return SLQ_OK;
}
extern "C" int slq_csr_affine_create(slq_context *ctx, int dtype, int64_t n, int64_t nnz_a, const int32_t *rp_a, const int32_t *ci_a,
                                     const void *va, int64_t nnz_b, const int32_t *rp_b, const int32_t *ci_b, const void *vb,
                                     slq_operator **out) {
  return create_guarded(out, [&]() { return csr_affine_create_body(ctx, dtype, n, nnz_a, rp_a, ci_a, va, nnz_b, rp_b, ci_b, vb, out); });
}

// t of an affine operator A + t B (SparseEigenAffineOperator::set_parameter, eigen_operators.h:134-136)
extern "C" int slq_operator_set_parameter(slq_operator *op, double t) {
  if (!op) return fail(SLQ_EINVAL, "op is NULL");
  if (op->kind == OP_KERNEL) return fail(SLQ_EINVAL, "a kernel operator has no parameter t: its hyperparameters are set by slq_kernel_set_parameters");
  if (op->kind == OP_KERNEL_PRECOND) return fail(SLQ_EINVAL, "a preconditioned kernel operator has no parameter t: set the hyperparameters of its base operator, then call slq_kernel_precond_refresh");
  if (op->kind == OP_TOEPLITZ) return fail(SLQ_EINVAL, "a Toeplitz operator has no parameter t: its values are set by slq_toeplitz_set_values");
  if (!op->vals_a || !op->vals_b) return fail(SLQ_EINVAL, "not an affine operator");
  HIP_TRY(hipSetDevice(op->ctx->device));
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(4096, (op->nnz + 255) / 256));
  if (op->dtype == SLQ_F64)
    k_affine_vals<double><<<grid, 256, 0, op->ctx->stream>>>(op->nnz, op->vals_a.as<const double>(), op->vals_b.as<const double>(), t, op->csr.vals.as<double>());
  else
    k_affine_vals<float><<<grid, 256, 0, op->ctx->stream>>>(op->nnz, op->vals_a.as<const float>(), op->vals_b.as<const float>(), t, op->csr.vals.as<float>());
  HIP_TRY(hipGetLastError());
  return SLQ_OK;
}

static int dense_create_body(slq_context *ctx, int dtype, int64_t n, const void *A, int64_t lda, slq_operator **out) {
  slq_operator *op = nullptr;
  SLQ_TRY(operator_new(ctx, OP_DENSE, dtype, n, n * n, out, &op));
  OpGuard guard{op};
  if (n <= 0 || n >= (int64_t)1 << 31 || !A || lda < n) return fail(SLQ_EINVAL, "bad dense operator shape");
  op->lda = n;
  const size_t es = esize(dtype);
  // Y = A X for whatever is given (eigen_operators.h:24-30 does not ask for symmetry either). k_dense_mfma_3term reads
  // A(row, k) and is right for any A; k_dense_panel walks row `row` of A as the contiguous COLUMN `row`, which is A^T:
  // equal for the symmetric operators Lanczos is meant for. An O(n^2) host pass checks that; a non-symmetric input
  // gets its transpose uploaded next to it for that kernel.
  bool symmetric = true;
  for (int64_t j = 0; j < n && symmetric; ++j)
    for (int64_t i = j + 1; i < n; ++i) {
      const bool same = dtype == SLQ_F64 ? ((const double *)A)[j * lda + i] == ((const double *)A)[i * lda + j]
                                         : ((const float *)A)[j * lda + i] == ((const float *)A)[i * lda + j];
      if (!same) { symmetric = false; break; }
    }
  hipError_t e = op->csr.vals.alloc((size_t)n * n * es);
  if (e == hipSuccess)
    e = hipMemcpy2DAsync(op->csr.vals.p, (size_t)n * es, A, (size_t)lda * es, (size_t)n * es, (size_t)n,
                         hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess && !symmetric) {
    std::vector<char> T((size_t)n * n * es);
    for (int64_t j = 0; j < n; ++j)
      for (int64_t i = 0; i < n; ++i)
        memcpy(T.data() + ((size_t)j * n + i) * es, (const char *)A + ((size_t)i * lda + j) * es, es);  // T(i,j) = A(j,i)
    e = op->dense_t.alloc((size_t)n * n * es);
    if (e == hipSuccess) e = hipMemcpyAsync(op->dense_t.p, T.data(), (size_t)n * n * es, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? SLQ_ENOMEM : SLQ_EHIP, "dense upload: %s", hipGetErrorString(e));
  *out = guard.release();
  return SLQ_OK;
}
extern "C" int slq_dense_create(slq_context *ctx, int dtype, int64_t n, const void *A, int64_t lda,
                                slq_operator **out) {
  return create_guarded(out, [&]() { return dense_create_body(ctx, dtype, n, A, lda, out); });
}

extern "C" int slq_callback_create(slq_context *ctx, int dtype, int64_t n, slq_matvec_fn fn,
                                   void *user, slq_operator **out) {
  slq_operator *op = nullptr;
  SLQ_TRY(operator_new(ctx, OP_CALLBACK, dtype, n, 0, out, &op));
  OpGuard guard{op};
  if (n <= 0 || n >= (int64_t)1 << 31) return fail(SLQ_EINVAL, "bad operator shape");
  if (!fn) return fail(SLQ_EINVAL, "Supplied object is missing 'matvec' attribute.");
  op->fn = fn, op->user = user;
  *out = guard.release();
  return SLQ_OK;
}

extern "C" int slq_device_callback_create(slq_context *ctx, int dtype, int64_t n, slq_matmat_device_fn fn, void *user,
                                          slq_operator **out) {
  if (!ctx || !out || !fn) return fail(SLQ_EINVAL, "ctx/out/fn is NULL");
  slq_operator *op = nullptr;
  SLQ_TRY(operator_new(ctx, OP_DEVICE_CALLBACK, dtype, n, 0, out, &op));
  OpGuard guard{op};
  if (n <= 0 || n >= (int64_t)1 << 31) return fail(SLQ_EINVAL, "bad operator size");
  op->dev_fn = fn, op->user = user;
  *out = guard.release();
  return SLQ_OK;
}

// ---- matrix-free kernel operator (slq_kernelop.hpp) ----
// z, |z|^2, s and sigma2 from the raw points and the operator's host record, on the library's stream (no allocation, no upload)
static int kernel_rescale(slq_operator *op) {
  HIP_TRY(op->k_pts.rescale(*op->k_scale, op->k_s, op->k_noise, op->dtype, op->ctx->stream));
  return SLQ_OK;
}
// a schedule as the array of the slq_debug_kernel*_schedule entries: the words of head (each entry has its own), then
// slab_begin[0 .. nslabs] and -1 up to max_slabs
static void kernel_schedule_words(std::initializer_list<int64_t> head, int nslabs, const int64_t *slab_begin, int max_slabs, int64_t *out) {
  out = std::copy(head.begin(), head.end(), out);
  for (int z = 0; z <= max_slabs; ++z) out[z] = z <= nslabs ? slab_begin[z] : -1;
}
// What the slq_debug_kernel*_schedule entries that write a KernelSchedule share: room for the words, the entry's own bounds on its
// arguments (args_ok; `bounds` says them), then the head - rows per block, row blocks, 16-column tiles per workgroup, column chunks,
// slabs and, of the products with a summed side of their own (head = 6), tiles per slab - and slab_begin. No HIP call.
static bool kernel_extents_ok(std::initializer_list<int64_t> extents, int num_cus) {
  return num_cus > 0 && std::all_of(extents.begin(), extents.end(), [](int64_t e) { return e > 0 && e < ((int64_t)1 << 31) - 16; });
}
template <typename Make>
static int kernel_schedule_debug(const char *who, bool args_ok, const char *bounds, int head, int max_slabs, int64_t *out, int nout, Make make) {
  if (!out || nout < head + max_slabs + 1) return fail(SLQ_EINVAL, "%s: room for %d values", who, head + max_slabs + 1);
  if (!args_ok) return fail(SLQ_EINVAL, "%s: %s", who, bounds);
  const KernelSchedule S = make();
  const int64_t words[6] = {S.rows_per_block, S.nrow_blocks, S.col_blocks, S.ncol_chunks, S.nslabs, S.tiles_per_slab};
  std::copy(words, words + head, out);
  kernel_schedule_words({}, S.nslabs, S.slab_begin, max_slabs, out + head);
  return SLQ_OK;
}
static int kernel_bad(const KernelBad &b) {
  char msg[256];
  kernel_bad_message(b, msg, sizeof msg);
  return fail(SLQ_EINVAL, "%s", msg);
}
static void kernel_set_scale(slq_operator *op, const double *ls, int nls, double s, double noise) {
  for (int k = 0; k < kKernelMaxDim; ++k) op->k_scale->ls[k] = k < op->k_pts.d ? ls[nls == 1 ? 0 : k] : 1.0;
  op->k_s = s, op->k_noise = noise;
}
static int kernel_create_body(slq_context *ctx, int dtype, int64_t n, int d, const void *points, int64_t ldp, int profile, const double *ls,
                              int nls, double s, double noise, bool on_device, slq_operator **out) {
  slq_operator *op = nullptr;
  SLQ_TRY(operator_new(ctx, OP_KERNEL, dtype, n, n * d, out, &op));
  OpGuard guard{op};
  if (!points || !ls) return fail(SLQ_EINVAL, "kernel operator: points/lengthscales is NULL");
  KernelBad bad = kernel_validate<double>(n, d, nullptr, ldp, profile, ls, nls, s, noise);  // (the points: below, on the host copy)
  if (bad.what != KERNEL_OK) return kernel_bad(bad);
  op->k_profile = profile;
  op->k_scale.reset(new KernelScale());
  for (int k = 0; k < kKernelMaxDim; ++k) op->k_scale->mean[k] = 0.0;
  const hipError_t e = op->k_pts.alloc_and_upload(n, d, points, ldp, on_device, dtype, ctx->stream, &bad, op->k_scale->mean);
  if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? SLQ_ENOMEM : SLQ_EHIP, "kernel operator upload: %s", hipGetErrorString(e));
  if (bad.what != KERNEL_OK) return kernel_bad(bad);
  // (the centre comes with the points' one host pass, so an overflowing mean is found after the allocation and the upload have been
  // issued: the guard's delete frees the buffer, and hipFree waits for the upload before the caller's points go away)
  for (int k = 0; k < d; ++k)
    if (!std::isfinite(op->k_scale->mean[k])) return fail(SLQ_EINVAL, "kernel operator: the mean of coordinate %d overflows", k);
  kernel_set_scale(op, ls, nls, s, noise);
  SLQ_TRY(kernel_rescale(op));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  *out = guard.release();
  return SLQ_OK;
}
extern "C" int slq_kernel_create(slq_context *ctx, int dtype, int64_t n, int d, const void *points, int64_t ldp, int profile,
                                 const double *lengthscales, int nls, double outputscale, double noise, slq_operator **out) {
  return create_guarded(out, [&]() { return kernel_create_body(ctx, dtype, n, d, points, ldp, profile, lengthscales, nls, outputscale, noise, false, out); });
}
extern "C" int slq_kernel_create_device(slq_context *ctx, int dtype, int64_t n, int d, const void *d_points, int64_t ldp, int profile,
                                        const double *lengthscales, int nls, double outputscale, double noise, slq_operator **out) {
  return create_guarded(out, [&]() { return kernel_create_body(ctx, dtype, n, d, d_points, ldp, profile, lengthscales, nls, outputscale, noise, true, out); });
}
extern "C" int slq_kernel_set_parameters(slq_operator *op, const double *lengthscales, int nls, double outputscale, double noise) {
  if (!op) return fail(SLQ_EINVAL, "op is NULL");
  if (op->kind == OP_KERNEL_PRECOND)
    return fail(SLQ_EINVAL, "slq_kernel_set_parameters: a preconditioned kernel operator takes its hyperparameters from its base operator: set them there, then call slq_kernel_precond_refresh");
  if (op->kind != OP_KERNEL) return fail(SLQ_EINVAL, "slq_kernel_set_parameters: not a kernel operator");
  const KernelBad bad = kernel_validate_parameters(op->k_pts.d, lengthscales, nls, outputscale, noise);
  if (bad.what != KERNEL_OK) return kernel_bad(bad);
  HIP_TRY(hipSetDevice(op->ctx->device));
  kernel_set_scale(op, lengthscales, nls, outputscale, noise);
  ++op->k_epoch;  // (cross objects re-derive their z* before their next product: slq_kernel_cross_*)
  return kernel_rescale(op);
}
extern "C" int slq_kernel_get_parameters(const slq_operator *op, int *d, int *profile, double *lengthscales, int nls, double *outputscale, double *noise) {
  if (!op) return fail(SLQ_EINVAL, "op is NULL");
  if (op->kind != OP_KERNEL) return fail(SLQ_EINVAL, "slq_kernel_get_parameters: not a kernel operator");
  if (lengthscales && nls != op->k_pts.d) return fail(SLQ_EINVAL, "slq_kernel_get_parameters: room for %d lengthscales, the operator has d = %d", nls, op->k_pts.d);
  if (d) *d = op->k_pts.d;
  if (profile) *profile = op->k_profile;
  if (lengthscales) std::copy(op->k_scale->ls, op->k_scale->ls + op->k_pts.d, lengthscales);
  if (outputscale) *outputscale = op->k_s;
  if (noise) *noise = op->k_noise;
  return SLQ_OK;
}
// what the product kernel reads, as it is on the device now: z transposed (dpad x npad, dpad = d rounded up to 4, npad = n rounded
// up to 16), |z|^2 (npad) and {s, sigma2}, in the operator's dtype (tests)
extern "C" int slq_debug_kernel_points(slq_operator *op, void *zt, void *nrm, void *params) {
  if (!op) return fail(SLQ_EINVAL, "op is NULL");
  if (op->kind != OP_KERNEL) return fail(SLQ_EINVAL, "slq_debug_kernel_points: not a kernel operator");
  HIP_TRY(hipSetDevice(op->ctx->device));
  HIP_TRY(hipStreamSynchronize(op->ctx->stream));
  HIP_TRY(op->k_pts.download(zt, nrm, params, op->dtype));
  return SLQ_OK;
}
// ---- the diagonal scale: A = s diag(c) phi(r2) diag(c) + sigma2 I ----
// The entries that are not built for a scaled operator ask here, at every use: the gradients, the preconditioner and everything on it.
static int kernel_refuse_scaled(const slq_operator *op, const char *who) {
  if (!op->k_scaled) return SLQ_OK;
  return fail(SLQ_EINVAL, "%s: the kernel operator has a diagonal scale (slq_kernel_set_diag_scale): this entry is not built for a scaled operator", who);
}
extern "C" int slq_kernel_set_diag_scale(slq_operator *op, const double *c, int64_t n) {
  if (!op) return fail(SLQ_EINVAL, "op is NULL");
  if (op->kind == OP_KERNEL_PRECOND)
    return fail(SLQ_EINVAL, "slq_kernel_set_diag_scale: a preconditioned kernel operator is not built for a diagonal scale");
  if (op->kind != OP_KERNEL) return fail(SLQ_EINVAL, "slq_kernel_set_diag_scale: not a kernel operator");
  if (!c) {  // clear: the operator is today's unscaled one again (the buffer stays where it is)
    if (op->k_scaled) ++op->k_epoch;
    op->k_scaled = false;
    op->k_c_host.clear();
    return SLQ_OK;
  }
  const bool f64 = op->dtype == SLQ_F64;
  const KernelBad bad = f64 ? kernel_validate_diag_scale<double>(op->n, c, n) : kernel_validate_diag_scale<float>(op->n, c, n);
  if (bad.what != KERNEL_OK) return kernel_bad(bad);
  HIP_TRY(hipSetDevice(op->ctx->device));
  return create_guarded(nullptr, [&]() {
    const size_t npad = (size_t)op->k_pts.npad;
    if (!op->k_c) {
      hipError_t e = op->k_c.alloc(npad * (f64 ? 8 : 4));
      if (e == hipSuccess) e = op->k_c_stage.alloc((size_t)op->n * 8);
      if (e != hipSuccess) {
        op->k_c.release(), op->k_c_stage.release();
        return fail(e == hipErrorOutOfMemory ? SLQ_ENOMEM : SLQ_EHIP, "slq_kernel_set_diag_scale: %s", hipGetErrorString(e));
      }
    }
    std::vector<double> rounded((size_t)op->n);
    for (size_t i = 0; i < rounded.size(); ++i) rounded[i] = f64 ? c[i] : (double)(float)c[i];
    hipStream_t st = op->ctx->stream;
    HIP_TRY(hipMemcpyAsync(op->k_c_stage.p, c, (size_t)op->n * 8, hipMemcpyHostToDevice, st));
    const dim3 g((unsigned)((npad + 255) / 256));
    if (f64) k_kernel_diag_scale<double><<<g, dim3(256), 0, st>>>((int)op->n, (int)npad, op->k_c_stage.as<const double>(), op->k_c.as<double>());
    else k_kernel_diag_scale<float><<<g, dim3(256), 0, st>>>((int)op->n, (int)npad, op->k_c_stage.as<const double>(), op->k_c.as<float>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));  // (the caller's c has been read when this returns)
    op->k_c_host.swap(rounded);
    op->k_scaled = true;
    ++op->k_epoch;
    return (int)SLQ_OK;
  });
}
extern "C" int slq_kernel_get_diag_scale(const slq_operator *op, double *c, int64_t n, int *is_set) {
  if (!op) return fail(SLQ_EINVAL, "op is NULL");
  if (op->kind != OP_KERNEL) return fail(SLQ_EINVAL, "slq_kernel_get_diag_scale: not a kernel operator");
  if (is_set) *is_set = op->k_scaled ? 1 : 0;
  if (c) {
    if (n != op->n) return fail(SLQ_EINVAL, "slq_kernel_get_diag_scale: room for %lld entries, the operator has n = %lld points", (long long)n, (long long)op->n);
    if (!op->k_scaled) return fail(SLQ_EINVAL, "slq_kernel_get_diag_scale: no diagonal scale is set (is_set reports it; pass c = NULL to ask)");
    std::copy(op->k_c_host.begin(), op->k_c_host.end(), c);
  }
  return SLQ_OK;
}
// the npad words of the scale as the product kernel reads them, in the operator's dtype (tests)
extern "C" int slq_debug_kernel_diag_scale(slq_operator *op, void *c_dev_words) {
  if (!op || !c_dev_words) return fail(SLQ_EINVAL, "slq_debug_kernel_diag_scale: op/c_dev_words is NULL");
  if (op->kind != OP_KERNEL) return fail(SLQ_EINVAL, "slq_debug_kernel_diag_scale: not a kernel operator");
  if (!op->k_scaled) return fail(SLQ_EINVAL, "slq_debug_kernel_diag_scale: no diagonal scale is set");
  HIP_TRY(hipSetDevice(op->ctx->device));
  HIP_TRY(hipStreamSynchronize(op->ctx->stream));
  HIP_TRY(hipMemcpy(c_dev_words, op->k_c.p, (size_t)op->k_pts.npad * (op->dtype == SLQ_F64 ? 8 : 4), hipMemcpyDeviceToHost));
  return SLQ_OK;
}
// kernel_schedule() of slq_kernelop.hpp as an array: rows per block, row blocks, 16-column tiles per workgroup, column chunks, slabs,
// then slab_begin[0 .. slabs]. No HIP call.
extern "C" int slq_debug_kernel_schedule(int64_t n, int panel_width, int panels, int num_cus, int64_t *out, int nout) {
  const bool ok = n > 0 && panel_width >= 16 && !(panel_width & (panel_width - 1)) && panels > 0 && num_cus > 0;
  return kernel_schedule_debug("slq_debug_kernel_schedule", ok, "n, panels, num_cus positive, panel_width a power of two >= 16", 5, kKernelMaxSlabs, out, nout,
                               [&]() { return kernel_schedule(n, panel_width, panels, num_cus); });
}

extern "C" int slq_operator_destroy(slq_operator *op) {
  if (!op) return SLQ_OK;
  hipSetDevice(op->ctx->device);
  slq_context *ctx = op->ctx;
  delete op;  // (every device array is a member that frees itself: slq_operator.hpp)
  ctx_release(ctx);
  return SLQ_OK;
}

// Tiles of R = 2 or 4 merged base tiles for the narrow-panel form of the ring-fed passes (slq_ring.hpp), built the first time
// a plan needs them and kept with the operator. A merged tile is R consecutive tiles of one XCD chunk - neighbours in the
// sweep, so most of what they read they share - with ONE line list (build_tile_meta on the merged row ranges), hence
// R x 14 rows, at most R x 36 lines and R x 112 nonzeros: exactly what a slot of that kernel holds. Everything comes
// from what the operator already keeps on the device (its CSR in stored order, the tile boundaries); nothing of the
// caller's is needed again. Returns false when the operator has no ring-sized tiles (or the build failed: the plan then
// takes the generic passes).
static bool ensure_ring_stream(slq_operator *op, int R) {
  const TileStreamPair &base = op->streams[0];
  if (R == 1) return (bool)base.full;
  if (!base.full || !op->tiles_ringed || (R != 2 && R != 4)) return false;
  TileStreamPair &m = op->streams[R == 2 ? 1 : 2];
  std::lock_guard<std::mutex> guard(op->merged_lock);
  if (m.tried) return (bool)m.full;
  m.tried = true;
  const int64_t n = op->n;
  const size_t es = esize(op->dtype);
  const int32_t ntiles = op->tiles.xcd_tile[8];
  const bool with_upper = base.upper && op->upper;
  const bool want_pad = op->sw.ring_pad_rows != 0;
  try {
    std::vector<int32_t> tr((size_t)ntiles + 1);
    if (hipMemcpy(tr.data(), op->tiles.tile_row.p, ((size_t)ntiles + 1) * 4, hipMemcpyDeviceToHost) != hipSuccess) return false;
    // merged tile boundaries, chunk by chunk (a merged tile never straddles two XCD chunks; a chunk's last one may be short)
    std::vector<int32_t> mrow;
    int32_t mxcd[9];
    for (int x = 0; x < 8; ++x) {
      mxcd[x] = (int32_t)mrow.size();
      for (int32_t t = op->tiles.xcd_tile[x]; t < op->tiles.xcd_tile[x + 1]; t += R) mrow.push_back(tr[(size_t)t]);
    }
    mxcd[8] = (int32_t)mrow.size();
    mrow.push_back((int32_t)n);
    std::copy(mxcd, mxcd + 9, m.full.xcd_tile);  // (known whether or not the build below succeeds)
    // the host's way (SLQ_DEVICE_BUILD=0, and the yardstick of SLQ_DEVICE_BUILD=2): the CSR comes back, lists and stream are built
    // here and uploaded
    auto build_host = [&](TileStreamPair &mm) -> bool {
      struct Fetched { std::vector<int32_t> rp, ci; std::vector<char> va; } F, FU;
      auto fetch = [&](const CsrArrays &c, Fetched &f) {
        f.rp.resize((size_t)n + 1), f.ci.resize((size_t)c.nnz), f.va.resize((size_t)c.nnz * es);
        return hipMemcpy(f.rp.data(), c.rowptr.p, f.rp.size() * 4, hipMemcpyDeviceToHost) == hipSuccess &&
               hipMemcpy(f.ci.data(), c.colind.p, f.ci.size() * 4, hipMemcpyDeviceToHost) == hipSuccess &&
               hipMemcpy(f.va.data(), c.vals.p, f.va.size(), hipMemcpyDeviceToHost) == hipSuccess;
      };
      HostStream hs, hsu;
      UploadQueue up(op->ctx->device);  // (declared after what it reads: joined first)
      bool ok = fetch(op->csr, F) && host_build_stream(op, R, HostCsr{F.rp.data(), F.ci.data(), F.va.data()}, mrow, false, 0.0, hs, up, mm.full) == hipSuccess && mm.full;
      if (ok && with_upper)
        ok = fetch(op->upper, FU) && host_build_stream(op, R, HostCsr{FU.rp.data(), FU.ci.data(), FU.va.data()}, mrow, want_pad, 0.0, hsu, up, mm.upper) == hipSuccess && mm.upper;
      return up.wait() == hipSuccess && ok;
    };
    // on the device (slq_build.hpp): the operator's CSR never leaves it
    auto build_device = [&](TileStreamPair &mm) -> bool {
      if (hipSetDevice(op->ctx->device) != hipSuccess) return false;
      DevBuf d_mrow;
      if (d_mrow.alloc(mrow.size() * 4) != hipSuccess) return false;
      if (hipMemcpy(d_mrow.p, mrow.data(), mrow.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return false;
      const int nm = (int)mrow.size() - 1;
      if (device_build_stream(op->ctx, op->dtype, R, n, op->csr.rp(), op->csr.ci(), op->csr.vals.p, d_mrow.as<int32_t>(), nm, false, 0.0, mm.full) != 0) return false;
      return !with_upper || device_build_stream(op->ctx, op->dtype, R, n, op->upper.rp(), op->upper.ci(), op->upper.vals.p, d_mrow.as<int32_t>(), nm, want_pad, 0.0, mm.upper) == 0;
    };
    // (a pair that failed half-way goes with everything it has: only a complete one reaches the operator)
    TileStreamPair built, ref;
    for (TileStreamPair *q : {&built, &ref}) {
      std::copy(mxcd, mxcd + 9, q->full.xcd_tile);
      if (with_upper) std::copy(mxcd, mxcd + 9, q->upper.xcd_tile);
    }
    const int dev_mode = op->sw.ring_order != 0 ? 0 : op->sw.device_build;  // (as the operator was built)
    if (!(dev_mode == 0 ? build_host(built) : build_device(built))) return false;
    if (dev_mode == 2 && (!build_host(ref) || streams_differ(ref.full, built.full) || streams_differ(ref.upper, built.upper))) {  // both, compared
      fprintf(stderr, "[slq] SLQ_DEVICE_BUILD=2: the device-built stream of %d-merged tiles differs from the host-built one\n", R);
      return false;
    }
    built.tried = true;
    m = std::move(built);
    return true;
  } catch (const std::bad_alloc &) {
    return false;
  }
}

// ---- Toeplitz operator (slq_toeplitz.hpp, slq_toeplitz.hip) ----
static int toeplitz_check_n(const char *who, int64_t n) {
  if (n < 1) return fail(SLQ_EINVAL, "%s: n = %lld must be at least 1", who, (long long)n);
  if (n > kToeplitzMaxN) return fail(SLQ_EINVAL, "%s: n = %lld exceeds the supported maximum %lld (L = 2^%d)", who, (long long)n, (long long)kToeplitzMaxN, kToeplitzMaxLog2L);
  return SLQ_OK;
}
// the symbol of (cr, rr) in double on the host, rounded to the dtype in the order the passes read it, into op->tz_sym on the
// context stream (the buffer exists and keeps its address); waits for the upload (the host words go with this frame)
template <typename F> static int toeplitz_upload_symbol(slq_operator *op, const std::vector<double> &cr, const std::vector<double> &rr) {
  const ToeplitzPlan P = toeplitz_plan(op->n, (int)sizeof(F), 16);
  const std::vector<std::complex<double>> s = toeplitz_symbol(P, cr, rr);
  std::vector<F> words((size_t)2 * P.L);
  toeplitz_device_symbol<F>(P, s, words.data());
  for (const F v : words)
    if (!std::isfinite(v)) return fail(SLQ_EINVAL, "Toeplitz operator: the symbol overflows the operator's dtype");
  HIP_TRY(hipMemcpyAsync(op->tz_sym.p, words.data(), words.size() * sizeof(F), hipMemcpyHostToDevice, op->ctx->stream));
  HIP_TRY(hipStreamSynchronize(op->ctx->stream));
  return SLQ_OK;
}
template <typename F> static int toeplitz_upload_tables(slq_operator *op) {
  const ToeplitzPlan P = toeplitz_plan(op->n, (int)sizeof(F), 16);
  hipStream_t st = op->ctx->stream;
  std::vector<F> tab((size_t)kToeplitzTab);
  toeplitz_device_tab<F>(tab.data());
  hipError_t e = op->tz_sym.alloc((size_t)2 * P.L * sizeof(F));
  if (e == hipSuccess) e = op->tz_tab.alloc(tab.size() * sizeof(F));
  if (e == hipSuccess) e = hipMemcpyAsync(op->tz_tab.p, tab.data(), tab.size() * sizeof(F), hipMemcpyHostToDevice, st);
  std::vector<F> tw[2];
  for (int j = 0; j + 1 < P.levels && e == hipSuccess; ++j) {
    const size_t count = (size_t)1 << (P.lg[j] + (int)toeplitz_level_stride_log2(P, j));
    tw[j].resize(2 * count);
    toeplitz_device_twiddles<F>(P, j, tw[j].data());
    e = op->tz_tw[j].alloc(2 * count * sizeof(F));
    if (e == hipSuccess) e = hipMemcpyAsync(op->tz_tw[j].p, tw[j].data(), 2 * count * sizeof(F), hipMemcpyHostToDevice, st);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? SLQ_ENOMEM : SLQ_EHIP, "Toeplitz operator upload: %s", hipGetErrorString(e));
  return SLQ_OK;
}
static int toeplitz_create_body(slq_context *ctx, int dtype, int64_t n, const double *c, const double *r, slq_operator **out) {
  if (!ctx || !out) return fail(SLQ_EINVAL, "ctx/out is NULL");
  *out = nullptr;
  SLQ_TRY(check_dtype(dtype));
  SLQ_TRY(toeplitz_check_n("slq_toeplitz_create", n));
  if (!c) return fail(SLQ_EINVAL, "slq_toeplitz_create: c is NULL");
  std::vector<double> cr, rr;
  bool sym = true;
  char msg[160];
  if (!toeplitz_round_values(n, (int)esize(dtype), c, r, cr, rr, &sym, msg, sizeof msg)) return fail(SLQ_EINVAL, "%s", msg);
  slq_operator *op = nullptr;
  SLQ_TRY(operator_new(ctx, OP_TOEPLITZ, dtype, n, 2 * n - 1, out, &op));
  OpGuard guard{op};
  if (!toeplitz_prepare()) return fail(SLQ_EHIP, "Toeplitz operator: the LDS limit of the product kernels could not be raised");
  SLQ_TRY(dtype == SLQ_F64 ? toeplitz_upload_tables<double>(op) : toeplitz_upload_tables<float>(op));
  SLQ_TRY(dtype == SLQ_F64 ? toeplitz_upload_symbol<double>(op, cr, rr) : toeplitz_upload_symbol<float>(op, cr, rr));
  op->tz_c = std::move(cr), op->tz_r = std::move(rr), op->tz_symmetric = sym;
  *out = guard.release();
  return SLQ_OK;
}
extern "C" int slq_toeplitz_create(slq_context *ctx, int dtype, int64_t n, const double *c, const double *r, slq_operator **out) {
  return create_guarded(out, [&]() { return toeplitz_create_body(ctx, dtype, n, c, r, out); });
}
extern "C" int slq_toeplitz_set_values(slq_operator *op, const double *c, const double *r, int64_t n) {
  if (!op || !c) return fail(SLQ_EINVAL, "slq_toeplitz_set_values: op/c is NULL");
  if (op->kind != OP_TOEPLITZ) return fail(SLQ_EINVAL, "slq_toeplitz_set_values: not a Toeplitz operator");
  if (n != op->n) return fail(SLQ_EINVAL, "slq_toeplitz_set_values: %lld values, the operator has n = %lld", (long long)n, (long long)op->n);
  try {
    std::vector<double> cr, rr;
    bool sym = true;
    char msg[160];
    if (!toeplitz_round_values(n, (int)esize(op->dtype), c, r, cr, rr, &sym, msg, sizeof msg)) return fail(SLQ_EINVAL, "%s", msg);
    if (sym != op->tz_symmetric)
      return fail(SLQ_EINVAL, "slq_toeplitz_set_values: the new values are %s, the operator is %s: a set may not change the symmetry (a live plan relies on it); create a new operator",
                  sym ? "symmetric" : "non-symmetric", op->tz_symmetric ? "symmetric" : "non-symmetric");
    HIP_TRY(hipSetDevice(op->ctx->device));
    SLQ_TRY(op->dtype == SLQ_F64 ? toeplitz_upload_symbol<double>(op, cr, rr) : toeplitz_upload_symbol<float>(op, cr, rr));
    op->tz_c = std::move(cr), op->tz_r = std::move(rr);
  } catch (const std::bad_alloc &) {
    return fail(SLQ_ENOMEM, "host allocation failed while computing the symbol");
  }
  return SLQ_OK;
}
extern "C" int slq_toeplitz_get_values(const slq_operator *op, double *c, double *r, int64_t n, int *symmetric) {
  if (!op) return fail(SLQ_EINVAL, "slq_toeplitz_get_values: op is NULL");
  if (op->kind != OP_TOEPLITZ) return fail(SLQ_EINVAL, "slq_toeplitz_get_values: not a Toeplitz operator");
  if ((c || r) && n != op->n) return fail(SLQ_EINVAL, "slq_toeplitz_get_values: room for %lld values, the operator has n = %lld", (long long)n, (long long)op->n);
  if (c) std::copy(op->tz_c.begin(), op->tz_c.end(), c);
  if (r) std::copy(op->tz_r.begin(), op->tz_r.end(), r);
  if (symmetric) *symmetric = op->tz_symmetric ? 1 : 0;
  return SLQ_OK;
}
// the pass structure of a product, without a device: out[0] L, [1] levels (1: one kernel, 2: three, 3: five), [2..4] the pass lengths
// L_1, L_2, L_3 (1 where unused), [5] LDS bytes of the largest kernel's workgroup, [6] complex columns of a workgroup, [7] workspace
// bytes of a plan (one panel in flight), [8] launches per panel, [9] the largest n supported
extern "C" int slq_debug_toeplitz_plan(int64_t n, int dtype, int panel_width, int64_t *out, int nout) {
  if (!out || nout < 10) return fail(SLQ_EINVAL, "slq_debug_toeplitz_plan: room for 10 values");
  SLQ_TRY(check_dtype(dtype));
  SLQ_TRY(toeplitz_check_n("slq_debug_toeplitz_plan", n));
  const int es = (int)esize(dtype);
  if (panel_width < 128 / es || panel_width > 1024 / es || (panel_width & (panel_width - 1)))  // (8 .. 64 lanes per row of 16 bytes)
    return fail(SLQ_EINVAL, "slq_debug_toeplitz_plan: panel_width = %d is not a panel width of the dtype", panel_width);
  const ToeplitzPlan P = toeplitz_plan(n, es, panel_width);
  out[0] = P.L, out[1] = P.levels;
  for (int j = 0; j < 3; ++j) out[2 + j] = j < P.levels ? (int64_t)1 << P.lg[j] : 1;
  out[5] = (int64_t)P.lds_bytes, out[6] = P.cg, out[7] = (int64_t)P.ws_bytes, out[8] = P.launches, out[9] = kToeplitzMaxN;
  return SLQ_OK;
}
// the symbol as the device holds it, brought back to natural order and to the scale of FFT_L(e): L complex numbers of the dtype (tests)
extern "C" int slq_debug_toeplitz_symbol(slq_operator *op, void *symbol_natural_order) {
  if (!op || !symbol_natural_order) return fail(SLQ_EINVAL, "slq_debug_toeplitz_symbol: op/symbol is NULL");
  if (op->kind != OP_TOEPLITZ) return fail(SLQ_EINVAL, "slq_debug_toeplitz_symbol: not a Toeplitz operator");
  HIP_TRY(hipSetDevice(op->ctx->device));
  HIP_TRY(hipStreamSynchronize(op->ctx->stream));
  const size_t es = esize(op->dtype);
  const ToeplitzPlan P = toeplitz_plan(op->n, (int)es, 16);
  try {
    std::vector<char> dev((size_t)2 * P.L * es);
    HIP_TRY(hipMemcpy(dev.data(), op->tz_sym.p, dev.size(), hipMemcpyDeviceToHost));
    for (int64_t pos = 0; pos < P.L; ++pos) {
      const int64_t k = toeplitz_freq_of(P, pos);
      for (int w = 0; w < 2; ++w) {
        if (es == 8) ((double *)symbol_natural_order)[2 * k + w] = ((const double *)dev.data())[2 * pos + w] * (double)P.L;
        else ((float *)symbol_natural_order)[2 * k + w] = ((const float *)dev.data())[2 * pos + w] * (float)P.L;
      }
    }
  } catch (const std::bad_alloc &) {
    return fail(SLQ_ENOMEM, "host allocation failed");
  }
  return SLQ_OK;
}

extern "C" int slq_debug_operator_device_bytes(int64_t *live) {
  if (!live) return fail(SLQ_EINVAL, "live is NULL");
  *live = g_devbuf_bytes.load();
  return SLQ_OK;
}

extern "C" int slq_operator_shape(const slq_operator *op, int64_t *nrows, int64_t *ncols,
                                  int64_t *nnz, int *dtype) {
  if (!op) return fail(SLQ_EINVAL, "op is NULL");
  if (nrows) *nrows = op->n;
  if (ncols) *ncols = op->n;
  if (nnz) *nnz = op->nnz;
  if (dtype) *dtype = op->dtype;
  return SLQ_OK;
}

// ---------------------------------------------------------------------------------------------------
// geometry + dispatch
// ---------------------------------------------------------------------------------------------------
template <int L> using LprTag = std::integral_constant<int, L>;
// calls fn(F{}, LprTag<L>{}) for the runtime (dtype, lanes-per-row) pair
template <typename Fn> static inline void dispatch(int dtype, int lpr, Fn &&fn) {
  if (dtype == SLQ_F64) {
    switch (lpr) {
      case 64: fn(double{}, LprTag<64>{}); break;
      case 32: fn(double{}, LprTag<32>{}); break;
      case 16: fn(double{}, LprTag<16>{}); break;
      default: fn(double{}, LprTag<8>{}); break;
    }
  } else {
    switch (lpr) {
      case 64: fn(float{}, LprTag<64>{}); break;
      case 32: fn(float{}, LprTag<32>{}); break;
      case 16: fn(float{}, LprTag<16>{}); break;
      default: fn(float{}, LprTag<8>{}); break;
    }
  }
}
#define DISPATCH(DT, LPRV, BODY)                          \
  dispatch(DT, LPRV, [&](auto _f, auto _l) {              \
    using F = decltype(_f);                               \
    constexpr int L = decltype(_l)::value;                \
    BODY;                                                 \
  })

static inline char *slot_ptr(const slq_plan *p, int slot) {
  return (char *)p->ring + (size_t)slot * (size_t)p->slot_stride * p->esz;
}

// profiling brackets ----------------------------------------------------------------------------------
static int prof_begin(slq_plan *p, int kind, ProfEvent *ev) {
  if (!p->prof) return SLQ_OK;
  if (!p->pool.empty()) {
    *ev = p->pool.back();
    p->pool.pop_back();
  } else {
    // no system-scope fence behind a record: nothing reads memory on the host behind these events (prof_collect
    // synchronises the stream first), and the cache writeback would be charged to the kernels around it
#ifdef SLQ_AB_EVENT_FENCE  // (A/B build: events with the fence)
    constexpr unsigned ev_flags = hipEventDefault;
#else
    constexpr unsigned ev_flags = hipEventDisableSystemFence;
#endif
    HIP_TRY(hipEventCreateWithFlags(&ev->a, ev_flags));
    HIP_TRY(hipEventCreateWithFlags(&ev->b, ev_flags));
  }
  ev->kind = kind;
  HIP_TRY(hipEventRecord(ev->a, p->ctx->stream));
  return SLQ_OK;
}
static int prof_end(slq_plan *p, ProfEvent *ev) {
  if (!p->prof) return SLQ_OK;
  HIP_TRY(hipEventRecord(ev->b, p->ctx->stream));
  p->events.push_back(*ev);
  return SLQ_OK;
}
#define PROFILED(plan, kind, launch)        \
  do {                                      \
    ProfEvent _ev;                          \
    SLQ_TRY(prof_begin(plan, kind, &_ev));  \
    launch;                                 \
    SLQ_TRY(prof_end(plan, &_ev));          \
  } while (0)

static int prof_collect(slq_plan *p) {
  if (p->events.empty()) return SLQ_OK;
  HIP_TRY(hipStreamSynchronize(p->ctx->stream));
  for (auto &ev : p->events) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
    p->acc.ms[ev.kind] += ms;
    p->acc.launches[ev.kind] += 1;
    p->pool.push_back(ev);
  }
  p->events.clear();
  return SLQ_OK;
}

extern "C" int slq_plan_profile_enable(slq_plan *plan, int enable) {
  if (!plan) return fail(SLQ_EINVAL, "plan is NULL");
  SLQ_TRY(prof_collect(plan));
  plan->prof = enable != 0;
  return SLQ_OK;
}

extern "C" int slq_plan_profile_read(slq_plan *plan, slq_profile *out, int reset) {
  if (!plan || !out) return fail(SLQ_EINVAL, "plan/out is NULL");
  HIP_TRY(hipSetDevice(plan->ctx->device));
  SLQ_TRY(prof_collect(plan));
  *out = plan->acc;
  if (reset) memset(&plan->acc, 0, sizeof(plan->acc));
  return SLQ_OK;
}

// ---------------------------------------------------------------------------------------------------
// plan
// ---------------------------------------------------------------------------------------------------
static int normalise_params(int64_t n, int *deg, int *orth) {
  if (*deg < 1) return fail(SLQ_EINVAL, "Number of steps must be positive!");
  if (*deg > n) *deg = (int)n;                                // lanczos.py:79, operators.py:68
  if (*deg > kMaxDeg) return fail(SLQ_EINVAL, "deg %d exceeds the supported maximum %d", *deg, kMaxDeg);
  if (*orth < 0 || *orth > *deg) *orth = *deg;                 // lanczos.py:88, operators.py:80
  return SLQ_OK;
}

// ||A||_inf of a CSR operator: the scale of one Lanczos step's rounding (what the edge recurrence adds to its noise radius per
// step). Taken once per operator, on the device, the first time a plan asks; affine operators change their values.
namespace slq {
template <typename F> __global__ void k_norm_inf(int n, const int32_t *__restrict__ rowptr, const F *__restrict__ vals, unsigned long long *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int32_t q = rowptr[i]; q < rowptr[i + 1]; ++q) s += fabs((double)vals[q]);
  atomicMax(out, (unsigned long long)__double_as_longlong(s));  // (bits of non-negative doubles order as integers)
}
}  // namespace slq
static int operator_norm_inf(slq_operator *op, double *out) {
  if (op->kind != OP_CSR || op->vals_b) return fail(SLQ_EINVAL, "no fixed CSR values to take ||A||_inf of");
  if (op->norm_inf < 0.0) {
    unsigned long long *d = nullptr, h = 0;
    hipStream_t st = op->ctx->stream;
    HIP_TRY(hipMalloc((void **)&d, 8));
    hipError_t e = hipMemsetAsync(d, 0, 8, st);
    if (e == hipSuccess) {
      const dim3 grid((unsigned)((op->n + 255) / 256));
      if (op->dtype == SLQ_F64) k_norm_inf<double><<<grid, 256, 0, st>>>((int)op->n, op->csr.rp(), op->csr.vals.as<const double>(), d);
      else k_norm_inf<float><<<grid, 256, 0, st>>>((int)op->n, op->csr.rp(), op->csr.vals.as<const float>(), d);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&h, d, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    hipFree(d);
    if (e != hipSuccess) return fail(SLQ_EHIP, "||A||_inf: %s", hipGetErrorString(e));
    double v;
    memcpy(&v, &h, 8);
    op->norm_inf = v;
  }
  *out = op->norm_inf;
  return SLQ_OK;
}

// The facts of a plan of `kind` on `op` (slq_plan_shape.hpp). No device work: the merged streams are reported as they are now
// (plan_create_mode builds the one its plan wants first).
static PlanFacts plan_facts_of(const slq_operator *op, int nprobes, int deg, int orth, PlanKind kind) {
  PlanFacts f;
  const TileStream &upper_stream = op->streams[0].upper;
  f.kind = op->kind, f.dtype = op->dtype, f.n = op->n, f.nnz = op->nnz, f.nnz_u = op->upper.nnz, f.upper = (bool)op->upper;
  f.mrows = op->kind == OP_KERNEL_PRECOND ? op->pre->rpad : op->mrows, f.lda = op->lda;
  f.has_tiles = (bool)op->tiles.tile_ptr, f.tiles_ringed = op->tiles_ringed, f.tiles_max_cols = op->tiles.max_cols;
  f.upper_per_row = op->upper_per_row, f.upper_stream = (bool)upper_stream, f.upper_padded = upper_stream.padded;
  f.far_per_row = op->far_per_row, f.affine = (bool)op->vals_b;
  std::copy(op->tiles.xcd_tile, op->tiles.xcd_tile + 9, f.xcd_tile);
  std::copy(upper_stream.xcd_tile, upper_stream.xcd_tile + 9, f.xcd_tile_u);
  {
    std::unique_lock<std::mutex> guard;
    if (op->tiles_ringed) guard = std::unique_lock<std::mutex>(op->merged_lock);  // (another plan's creation may be building one)
    for (int i = 0; i < 2; ++i) {
      const TileStreamPair &m = op->streams[1 + i];
      f.merged[i].available = (bool)m.full, f.merged[i].upper = (bool)m.upper, f.merged[i].u_padded = m.upper.padded;
      std::copy(m.full.xcd_tile, m.full.xcd_tile + 9, f.merged[i].xcd_tile);
    }
  }
  f.num_cus = op->ctx->num_cus;
  f.nprobes = nprobes, f.deg = deg, f.orth = orth, f.plan = kind;
  return f;
}

static int check_query(int dtype, int64_t n, int nprobes, size_t *bytes) {
  if (!bytes) return fail(SLQ_EINVAL, "bytes is NULL");
  SLQ_TRY(check_dtype(dtype));
  if (n <= 0 || nprobes <= 0) return fail(SLQ_EINVAL, "n and nprobes must be positive");
  return SLQ_OK;
}
// the ring region of the shape of a plan that exists only as (dtype, n, nprobes, deg, orth, kind): the region depends on nothing else
static size_t query_ring_bytes(int dtype, int64_t n, int nprobes, int deg, int orth, PlanKind kind) {
  PlanFacts f;
  f.dtype = dtype, f.n = n, f.nprobes = nprobes, f.deg = deg, f.orth = orth, f.plan = kind;
  return plan_shape(f, read_plan_switches()).ws[WS_RING].bytes;
}

extern "C" int slq_plan_query_bytes(int dtype, int64_t n, int nprobes, int deg, int orth,
                                    int keep_basis, size_t *bytes) {
  SLQ_TRY(check_query(dtype, n, nprobes, bytes));
  SLQ_TRY(normalise_params(n, &deg, &orth));
  *bytes = query_ring_bytes(dtype, n, nprobes, deg, orth, keep_basis ? PlanKind::KeepBasis : PlanKind::Ring);
  return SLQ_OK;
}

// The footprint of a recompute plan does not depend on deg once deg > kAccCols, so the query answers for any deg >= 1 (a plan
// itself is still limited to kMaxDeg steps).
extern "C" int slq_plan_query_bytes_recompute(int dtype, int64_t n, int nprobes, int deg, int orth, size_t *bytes) {
  SLQ_TRY(check_query(dtype, n, nprobes, bytes));
  if (deg < 1) return fail(SLQ_EINVAL, "Number of steps must be positive!");
  if (deg > n) deg = (int)n;
  if (orth < 0 || orth > deg) orth = deg;
  *bytes = query_ring_bytes(dtype, n, nprobes, deg, orth, PlanKind::Recompute);  // (with the stash of the probes and the output panel)
  return SLQ_OK;
}

// What a plan of a kind (basis_mode 0 ring only, 1 kept basis, 2 recompute) on `op` allocates, for the one-shot entries, which
// size their probe chunks from it: plan_estimate_bytes (slq_plan_shape.hpp) - a bound, not the exact footprint.
static int plan_bytes_on_mode(const slq_operator *op, int nprobes, int deg, int orth, int mode, size_t *bytes) {
  SLQ_TRY(check_query(op->dtype, op->n, nprobes, bytes));
  SLQ_TRY(normalise_params(op->n, &deg, &orth));
  const PlanFacts f = plan_facts_of(op, nprobes, deg, orth, mode == 2 ? PlanKind::Recompute : (mode == 1 ? PlanKind::KeepBasis : PlanKind::Ring));
  *bytes = plan_estimate_bytes(plan_shape(f, read_plan_switches()), f);
  return SLQ_OK;
}
static int plan_bytes_on(const slq_operator *op, int nprobes, int deg, int orth, int keep_basis, size_t *bytes) {
  return plan_bytes_on_mode(op, nprobes, deg, orth, keep_basis ? 1 : 0, bytes);
}

extern "C" int slq_plan_destroy(slq_plan *p) {
  if (!p) return SLQ_OK;
  hipSetDevice(p->ctx->device);
  drop_closing_tail(p);  // (a pending closing tail goes with the plan: nothing is launched)
  hipStreamSynchronize(p->ctx->stream);
  for (auto &ev : p->events) { hipEventDestroy(ev.a); hipEventDestroy(ev.b); }
  for (auto &ev : p->pool) { hipEventDestroy(ev.a); hipEventDestroy(ev.b); }
  for (auto &g : p->graphs) hipGraphExecDestroy(g.exec);
  if (p->replay_exec) hipGraphExecDestroy(p->replay_exec);
  // what later calls allocated on demand
  if (p->at_d) hipFree(p->at_d);
  if (p->at_flags) hipFree(p->at_flags);
  if (p->om_ticket) hipFree(p->om_ticket);
  if (p->stage) hipFree(p->stage);
  // the workspace table (plan_materialise)
  for (void *q : p->ws)
    if (q) hipFree(q);
  ctx_release(p->ctx);
  delete p;
  return SLQ_OK;
}

static int set_kernel_attributes(slq_plan *p);
static seq::SequenceFacts sequence_facts(const slq_plan *p);

static int plan_create_mode(slq_context *ctx, slq_operator *op, int nprobes, int deg, int orth, PlanKind kind, slq_plan **out, bool product_only = false);

extern "C" int slq_plan_create(slq_context *ctx, slq_operator *op, int nprobes, int deg, int orth,
                               int keep_basis, slq_plan **out) {
  return plan_create_mode(ctx, op, nprobes, deg, orth, keep_basis != 0 ? PlanKind::KeepBasis : PlanKind::Ring, out);
}

extern "C" int slq_plan_create_recompute(slq_context *ctx, slq_operator *op, int nprobes, int deg, int orth, slq_plan **out) {
  return plan_create_mode(ctx, op, nprobes, deg, orth, PlanKind::Recompute, out);
}

extern "C" int slq_plan_basis_mode(const slq_plan *p, int *mode, int *ring_slots_out, int *acc_cols) {
  if (!p) return fail(SLQ_EINVAL, "plan is NULL");
  if (mode) *mode = p->basis_mode;
  if (ring_slots_out) *ring_slots_out = p->S;
  if (acc_cols) *acc_cols = p->acc_cols;
  return SLQ_OK;
}

// the plan's fields that repeat its shape (what the launchers read), and the tile stream the shape chose as pointers
static void plan_adopt_shape(slq_plan *p) {
  const PlanFacts &f = p->facts;
  const PlanShape &sh = p->shape;
  const slq_operator *op = p->op;
  p->cheb = is_cheb(f.plan);
  p->cheb_action = f.plan == PlanKind::ChebyshevAction;
  p->basis_mode = basis_mode_of(f.plan);
  p->keep_basis = f.plan == PlanKind::KeepBasis;
  p->dtype = op->dtype, p->n = (int)op->n, p->nprobes = f.nprobes, p->deg = f.deg, p->orth = f.orth;
  p->esz = esize(op->dtype);
  p->LPR = sh.LPR, p->PW = sh.PW, p->NP = sh.NP, p->bpad = sh.bpad, p->S = sh.S;
  p->acc_cols = sh.acc_cols, p->v_slot = sh.v_slot, p->y_slot = sh.y_slot;
  p->slot_stride = sh.slot_stride, p->rmax = sh.rmax;
  p->pipelined = sh.pipelined != 0;
  p->nblkA = sh.nblkA, p->nblkS = sh.nblkS, p->nblkU = sh.nblkU, p->nblkF = sh.nblkF, p->nblkT = sh.nblkT;
  p->alpha_pad = sh.alpha_pad, p->part_maxblk = sh.part_maxblk, p->dense_ks = sh.dense_ks;
  p->ringR = sh.ringR, p->ring_staged = sh.ring_staged != 0;
  p->rs_full = p->rs_upper = nullptr;
  if (sh.stream != STREAM_NONE) {
    const TileStreamPair &m = op->streams[sh.stream - STREAM_BASE];
    p->rs_full = &m.full;
    // (the base stream's upper half only where the shape takes it; a merged pair's whenever it has one)
    if (m.upper && (sh.stream != STREAM_BASE || sh.rs_upper)) p->rs_upper = &m.upper;
  }
  p->ring_gen = sh.seq.ring_gen, p->ring_deep = sh.seq.ring_deep, p->gram = sh.seq.gram, p->gram_csr = sh.seq.gram_csr, p->last_nostore = sh.seq.last_nostore;
  p->omega_on = sh.omega_on != 0;
  p->acc_skip = p->sw.acc_skip != 0;
  p->sweep_skip = p->sw.sweep_skip != 0;
  p->nstale = 0;
}

// allocates the shape's workspace table, clears what it marks, sets the kernel attributes and takes the operator's norm. On
// failure the plan is left for slq_plan_destroy, which frees whatever the table had allocated.
static int plan_materialise(slq_plan *p) {
  const PlanShape &sh = p->shape;
  hipError_t e = hipSuccess;
  for (const Region &r : sh.ws) {
    if (e != hipSuccess || !r.bytes) continue;
    e = hipMalloc(&p->ws[r.id], r.bytes);
    if (e == hipSuccess && r.zeroed == 1) e = hipMemset(p->ws[r.id], 0, r.bytes);
  }
  if (e != hipSuccess)
    return fail(e == hipErrorOutOfMemory ? SLQ_ENOMEM : SLQ_EHIP, "plan workspace (%zu bytes of Lanczos panels): %s", sh.ws[WS_RING].bytes, hipGetErrorString(e));
  p->ring = p->ws[WS_RING], p->scal = (double *)p->ws[WS_SCAL], p->part = (double *)p->ws[WS_PART], p->acc_coef = (double *)p->ws[WS_ACC_COEF];
  p->sweep_cols_d = (unsigned long long *)p->ws[WS_SWEEP_COLS];
  p->om_buf = (double *)p->ws[WS_OM_BUF], p->om_flags = (int *)p->ws[WS_OM_FLAGS], p->om_cnt = (unsigned long long *)p->ws[WS_OM_CNT];
  p->om_census = (int *)p->ws[WS_OM_CENSUS];
  p->quad_d = (double *)p->ws[WS_QUAD];
  p->cheb_mu = (double *)p->ws[WS_CHEB_MU], p->cheb_out = (int *)p->ws[WS_CHEB_OUT], p->cheb_coef = (double *)p->ws[WS_CHEB_COEF];
  p->T = p->ws[WS_T], p->T2 = p->ws[WS_T2];
  const ScalOffsets &so = sh.scal;
  double *const s = p->scal;
  p->st.alpha = s + so.alpha, p->st.nu = s + so.nu, p->st.vnorm2 = s + so.vnorm2, p->st.coefA = s + so.coefA, p->st.coefB = s + so.coefB;
  p->st.cross = s + so.cross, p->st.gram = s + so.gram, p->st.gamma = s + so.gamma;
  p->st.active = (int *)p->ws[WS_ACTIVE];
  p->st.steps = p->st.active + sh.active.steps;
  p->fail_d = p->st.active + sh.active.fail;
  p->ring_fail_d = p->st.active + sh.active.ring_fail;  // raised by k_csr_ring_pass when a bounded spin ran out (never cleared: the plan is dead)
  if (hipMemset(p->ring_fail_d, 0, 2 * sizeof(int)) != hipSuccess) return fail(SLQ_EHIP, "hipMemset failed");  // (and fail_d[2]: the QL status of a density update)
  p->st.bpad = p->bpad;
  p->st.nprobes = p->nprobes;
  p->st.deg = p->deg;
  p->nodes_d = p->quad_d + sh.bpad;
  p->weights_d = p->nodes_d + (size_t)sh.bpad * (size_t)sh.hist;
  for (const Region &r : sh.ws) {
    if (r.zeroed != 2 || !r.bytes) continue;
    const hipError_t ze = hipMemsetAsync(p->ws[r.id], 0, r.bytes, p->ctx->stream);
    if (ze != hipSuccess) return fail(SLQ_EHIP, "workspace clear: %s", hipGetErrorString(ze));
  }
  SLQ_TRY(set_kernel_attributes(p));
  if (p->omega_on) {
    SLQ_TRY(operator_norm_inf(p->op, &p->om_norm));
    hipError_t te = hipMalloc((void **)&p->om_ticket, (size_t)p->NP * sizeof(int));
    if (te == hipSuccess) te = hipMemset(p->om_ticket, 0, (size_t)p->NP * sizeof(int));
    if (te != hipSuccess) return fail(SLQ_EHIP, "rescue tickets: %s", hipGetErrorString(te));
  }
  return SLQ_OK;
}

// product_only: the two-slot plan of slq_operator_matmat, which runs no recurrence (the one plan a non-symmetric Toeplitz operator gets)
static int plan_create_mode(slq_context *ctx, slq_operator *op, int nprobes, int deg, int orth, PlanKind kind, slq_plan **out, bool product_only) {
  if (!ctx || !op || !out) return fail(SLQ_EINVAL, "ctx/op/out is NULL");
  *out = nullptr;
  if (op->ctx != ctx) return fail(SLQ_EINVAL, "operator belongs to another context");
  if (op->kind == OP_TOEPLITZ && !op->tz_symmetric && !product_only)
    return fail(SLQ_EINVAL, "the Toeplitz operator is non-symmetric (r differs from c): Lanczos and Chebyshev plans need a symmetric operator; slq_operator_matmat computes its products");
  if (nprobes <= 0) return fail(SLQ_EINVAL, "nprobes must be positive");
  // a Chebyshev plan: deg steps of the orth-0 geometry, bounded by kMaxChebSteps (neither by n nor by kMaxDeg: nothing is orthogonalised or diagonalised)
  if (is_cheb(kind) && (deg < 1 || deg > kMaxChebSteps)) return fail(SLQ_EINVAL, "slq_plan_create_chebyshev: nsteps = %d must lie in [1, %d]", deg, kMaxChebSteps);
  if (!is_cheb(kind)) SLQ_TRY(normalise_params(op->n, &deg, &orth));
  HIP_TRY(hipSetDevice(ctx->device));
  if (ctx->dead) return fail(SLQ_EINVAL, "the context has been destroyed");
  slq_plan *p = new (std::nothrow) slq_plan();
  if (!p) return fail(SLQ_ENOMEM, "host allocation failed");
  p->ctx = ctx;
  ctx_retain(ctx);
  p->op = op;
  p->sw = read_plan_switches();  // (the one read of this plan: nothing below, and nothing the plan does later, looks at the environment)
  // the merged tiles of narrow panels are built on first use - device work, so before the facts are taken
  if (const int R = wants_merged_stream(plan_facts_of(op, nprobes, deg, orth, kind), p->sw)) ensure_ring_stream(op, R);
  p->facts = plan_facts_of(op, nprobes, deg, orth, kind);
  p->shape = plan_shape(p->facts, p->sw);
  plan_adopt_shape(p);
  const int rc = plan_materialise(p);
  if (rc != SLQ_OK) {
    slq_plan_destroy(p);
    return rc;
  }
  *out = p;
  return SLQ_OK;
}

// plan_shape() of slq_plan_shape.hpp on facts given as an array (the order of plan_facts_to_array), the answer as an array (the
// order of plan_shape_to_array, workspace table included), under the switches as a creation would read them now: no HIP call, so
// that a CPU test enumerates the decision
extern "C" int slq_debug_plan_shape(const double *facts, int nfacts, double *out, int nout) {
  if (!facts || !out || nfacts != kNumPlanFacts || nout != kNumPlanShape)
    return fail(SLQ_EINVAL, "slq_debug_plan_shape: %d facts in, %d values out", kNumPlanFacts, kNumPlanShape);
  const PlanFacts f = plan_facts_from_array(facts);
  // (OP_KERNEL is not taken here: its shape is that of a callback operator plus the j slabs of slq_debug_kernel_schedule, and a live
  // plan answers through slq_debug_plan_shape_of)
  if (f.kind < OP_CSR || f.kind > OP_GRAM || (f.dtype != kF32 && f.dtype != kF64) || (int)f.plan < 0 || (int)f.plan > (int)PlanKind::ChebyshevAction)
    return fail(SLQ_EINVAL, "slq_debug_plan_shape: operator kind, dtype or plan kind out of range");
  if (f.n <= 0 || f.nprobes <= 0 || f.deg < 1 || f.orth < 0 || f.num_cus <= 0) return fail(SLQ_EINVAL, "slq_debug_plan_shape: n, nprobes, deg, num_cus must be positive");
  plan_shape_to_array(plan_shape(f, read_plan_switches()), out);
  return SLQ_OK;
}
// the facts and the shape a live plan was created from, in the same orders
extern "C" int slq_debug_plan_shape_of(const slq_plan *p, double *facts_out, int nfacts, double *shape_out, int nout) {
  if (!p || !facts_out || !shape_out || nfacts != kNumPlanFacts || nout != kNumPlanShape)
    return fail(SLQ_EINVAL, "slq_debug_plan_shape_of: plan, %d facts out, %d values out", kNumPlanFacts, kNumPlanShape);
  plan_facts_to_array(p->facts, facts_out);
  plan_shape_to_array(p->shape, shape_out);
  return SLQ_OK;
}

// Kernels that may be launched with more than the default 64 KiB of dynamic LDS (gamma staging): raise their limit once,
// outside any stream capture. Taking a kernel's address instantiates it, so these enumerations are also part of what decides
// which kernels the library contains: every (pass, load policy, ring columns, pipelined) combination a launcher can name.
template <int... I, typename Fn> static inline void for_each_int(std::integer_sequence<int, I...>, Fn &&fn) {
  (fn(std::integral_constant<int, I>{}), ...);
}
// fn(kernel) for every k_csr_pass<F, L, PASS, NTP, RC, PIPE> of the library: ALPHA has no ring columns, DOTS / ADOTS / UPDATEG
// at least one, UPDATEG the nontemporal form only; the pipelined row loop exists for 64 lanes per row, and not for ALPHA
template <typename F, int L, typename Fn> static inline void for_each_csr_pass(Fn &&fn) {
  for_each_int(std::integer_sequence<int, PASS_ALPHA, PASS_DOTS, PASS_ADOTS, PASS_UPDATE, PASS_UPDATEG>{}, [&](auto pass) {
    for_each_int(std::make_integer_sequence<int, 2>{}, [&](auto ntp) {
      for_each_int(std::make_integer_sequence<int, kFusedMaxR + 1>{}, [&](auto rc) {
        for_each_int(std::make_integer_sequence<int, 2>{}, [&](auto pipe) {
          constexpr int P = decltype(pass)::value, NTP = decltype(ntp)::value, RC = decltype(rc)::value, PIPE = decltype(pipe)::value;
          constexpr bool rc_ok = P == PASS_ALPHA ? RC == 0 : (P == PASS_UPDATE || RC >= 1);
          if constexpr (rc_ok && (P != PASS_UPDATEG || NTP == 1) && (PIPE == 0 || (L == 64 && P != PASS_ALPHA)))
            fn((const void *)k_csr_pass<F, L, P, NTP, RC, PIPE>);
        });
      });
    });
  });
}
// ... and for every k_csr_tile_pass (MAXRC = kFusedMaxR) / k_csr_ring_pass (MAXRC = kRingMaxR, and the SPMM pass): ALPHA,
// UPDATE (and SPMM) without ring columns, ADOTS and UPDATE with 1 .. MAXRC
template <typename F, bool RING, typename Fn> static inline void for_each_tiled_pass(Fn &&fn) {
  constexpr int MAXRC = RING ? kRingMaxR : kFusedMaxR;
  for_each_int(std::integer_sequence<int, PASS_ALPHA, PASS_UPDATE, PASS_SPMM, PASS_ADOTS>{}, [&](auto pass) {
    for_each_int(std::make_integer_sequence<int, 2>{}, [&](auto ntp) {
      for_each_int(std::make_integer_sequence<int, MAXRC + 1>{}, [&](auto rc) {
        constexpr int P = decltype(pass)::value, NTP = decltype(ntp)::value, RC = decltype(rc)::value;
        constexpr bool rc_ok = P == PASS_UPDATE || (P == PASS_ADOTS ? RC >= 1 : RC == 0);
        if constexpr (rc_ok && (P != PASS_SPMM || RING)) {
          if constexpr (RING) fn((const void *)k_csr_ring_pass<F, P, NTP, RC>);
          else fn((const void *)k_csr_tile_pass<F, P, NTP, RC>);
        }
      });
    });
  });
}
template <typename F, int L> static hipError_t raise_lds_limits() {
  hipError_t e = hipSuccess;
  auto raise = [&e](const void *fn) {
    if (e == hipSuccess) e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  };
  raise((const void *)k_reorth_update<F, L>);
  // fused passes: LDS padding caps their residency (SLQ_ALPHA_LDS_PAD experiments; dots/update: 2 per CU)
  for_each_csr_pass<F, L>(raise);
  if constexpr (L == 64) {
    for_each_tiled_pass<F, false>(raise);
    for_each_tiled_pass<F, true>(raise);
  }
  return e;
}
static int set_kernel_attributes(slq_plan *p) {
  hipError_t ae = hipSuccess;
  DISPATCH(p->dtype, p->LPR, (ae = raise_lds_limits<F, L>()));
  HIP_TRY(ae);
  if (p->ring_gen || p->ring_deep) {
    hipError_t re = hipSuccess;
    const bool d = p->dtype == SLQ_F64;
    switch (p->LPR) {
      case 64: re = d ? slq_ring_prepare_f64_l64() : slq_ring_prepare_f32_l64(); break;
      case 32: re = d ? slq_ring_prepare_f64_l32() : slq_ring_prepare_f32_l32(); break;
      default: re = d ? slq_ring_prepare_f64_l16() : slq_ring_prepare_f32_l16(); break;
    }
    HIP_TRY(re);
  }
  // (never from inside a stream capture: launch_dense_mfma runs under one)
  HIP_TRY(hipFuncSetAttribute((const void *)k_dense_mfma_3term<16>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  HIP_TRY(hipFuncSetAttribute((const void *)k_dense_mfma_3term<32>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  HIP_TRY(hipFuncSetAttribute((const void *)k_dense_mfma_3term<64>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));

  return SLQ_OK;
}

// the plan's fused passes run on the operator's workgroup tiles (slq_plan_create decides: wide panels, and narrow ones of the ring-fed form)
static bool plan_tiled(const slq_plan *p) { return p->ringR > 0; }

// k_csr_ring_pass raises *ring_fail_d when one of its bounded waits ran out (slq_kernels.hpp: kRingSpinMax): everything the
// plan holds is then undefined. ring_flag_status() is the flag -> status translation (no HIP call in it: a CPU test covers
// it through slq_debug_ring_flag_status); check_ring_flag() reads the device word behind whatever the caller has enqueued
// and is called by EVERY accessor that hands results of a run to the host.
static int ring_flag_status(int flag) {
  if (flag) return fail(SLQ_EHIP, "the ring-fed tile pass gave up waiting on a tile (SLQ_TILES=2): results are invalid");
  return SLQ_OK;
}
static int check_ring_flag(slq_plan *p) {
  int flag = 0;
  HIP_TRY(hipMemcpyAsync(&flag, p->ring_fail_d, sizeof(int), hipMemcpyDeviceToHost, p->ctx->stream));
  HIP_TRY(hipStreamSynchronize(p->ctx->stream));
  return ring_flag_status(flag);
}
extern "C" int slq_debug_ring_flag_status(int flag) { return ring_flag_status(flag); }
// test hook: set the plan's device flag as an aborting workgroup would (tests/test_gpu_api.py)
extern "C" int slq_debug_plan_poke_ring_flag(slq_plan *p, int value) {
  if (!p) return fail(SLQ_EINVAL, "plan is NULL");
  HIP_TRY(hipSetDevice(p->ctx->device));
  HIP_TRY(hipMemcpyAsync(p->ring_fail_d, &value, sizeof(int), hipMemcpyHostToDevice, p->ctx->stream));
  HIP_TRY(hipStreamSynchronize(p->ctx->stream));
  return SLQ_OK;
}

extern "C" int slq_plan_describe(const slq_plan *p, slq_plan_info *out) {
  if (!p || !out) return fail(SLQ_EINVAL, "plan/out is NULL");
  memset(out, 0, sizeof(*out));  // (and the retired trailing field stays 0: include/slq.h)
  out->panel_width = p->PW;
  out->panels = p->NP;
  out->ring_slots = p->S;
  out->sequence = seq::plan_sequence_of(sequence_facts(p));
  out->pipelined = p->pipelined ? 1 : 0;
  out->reordered = p->op->perm_d ? 1 : 0;
  out->upper_alpha = p->op->upper ? 1 : 0;
  out->far_per_row = p->op->far_per_row;
  out->tiles = plan_tiled(p) ? (p->op->tiles_ringed ? 2 : 1) : 0;
  return SLQ_OK;
}

// Byte accounting of the store-and-revisit update sweep, which reads a ring column only when SOME probe of the panel projects on it (k_reorth_update): how many
// columns it read and how many it was offered, summed over launches and panels since the last reset. Synchronises.
extern "C" int slq_plan_sweep_columns(slq_plan *p, uint64_t *read, uint64_t *offered, int reset) {
  if (!p) return fail(SLQ_EINVAL, "plan is NULL");
  HIP_TRY(hipSetDevice(p->ctx->device));
  unsigned long long h[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(h, p->sweep_cols_d, sizeof(h), hipMemcpyDeviceToHost, p->ctx->stream));
  if (reset) HIP_TRY(hipMemsetAsync(p->sweep_cols_d, 0, sizeof(h), p->ctx->stream));
  HIP_TRY(hipStreamSynchronize(p->ctx->stream));
  if (read) *read = h[0];
  if (offered) *offered = h[1];
  return SLQ_OK;
}

// The edge recurrence's accounting, summed over steps and panels since the last reset: oldest window columns
// offered, read, rescues (the entry measured after all by a dot of its own), verify-mode violations, read -> skip transitions.
// A plan that offers nothing reports zeros. Synchronises.
extern "C" int slq_plan_window_columns(slq_plan *p, int64_t out[5], int reset) {
  if (!p || !out) return fail(SLQ_EINVAL, "plan/out is NULL");
  for (int k = 0; k < 5; ++k) out[k] = 0;
  if (!p->omega_on) return SLQ_OK;
  HIP_TRY(hipSetDevice(p->ctx->device));
  SLQ_TRY(flush_closing_tail(p));  // (k_fin_beta_gram counts the closing step)
  unsigned long long h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(h, p->om_cnt, sizeof(h), hipMemcpyDeviceToHost, p->ctx->stream));
  if (reset) HIP_TRY(hipMemsetAsync(p->om_cnt, 0, sizeof(h), p->ctx->stream));
  HIP_TRY(hipStreamSynchronize(p->ctx->stream));
  for (int k = 0; k < 5; ++k) out[k] = (int64_t)h[k];
  return SLQ_OK;
}

// The flags of the last run (diagnostics, tests): read[j * panels + panel] / rescue[...] = 1 where the panel's update pass of step j read the window's
// oldest column / where its entry was measured by the rescue kernel; rows of steps that were not offered are zero. len = (deg + 1) * panels.
extern "C" int slq_plan_window_flags(slq_plan *p, int32_t *read, int32_t *rescue, int64_t len) {
  if (!p || !read || !rescue) return fail(SLQ_EINVAL, "plan/read/rescue is NULL");
  const int64_t words = (int64_t)(p->deg + 1) * p->NP;
  if (len != words) return fail(SLQ_EINVAL, "flag buffers: %lld words expected", (long long)words);
  memset(read, 0, (size_t)words * sizeof(int32_t));
  memset(rescue, 0, (size_t)words * sizeof(int32_t));
  if (!p->omega_on) return SLQ_OK;
  HIP_TRY(hipSetDevice(p->ctx->device));
  SLQ_TRY(flush_closing_tail(p));
  HIP_TRY(hipMemcpyAsync(read, p->om_flags, (size_t)words * sizeof(int), hipMemcpyDeviceToHost, p->ctx->stream));
  HIP_TRY(hipMemcpyAsync(rescue, p->om_flags + words, (size_t)words * sizeof(int), hipMemcpyDeviceToHost, p->ctx->stream));
  HIP_TRY(hipStreamSynchronize(p->ctx->stream));
  return SLQ_OK;
}

// Verify-mode census of the last run (any ring-fed Gram plan created under SLQ_OMEGA=2): out[(j * 9 + i) * panels + panel] = probes of the
// panel with a non-zero gamma at window position i of step j; len = (deg + 1) * 9 * panels words. Synchronises.
extern "C" int slq_plan_window_census(slq_plan *p, int32_t *out, int64_t len) {
  if (!p || !out) return fail(SLQ_EINVAL, "plan/out is NULL");
  const int64_t words = (int64_t)(p->deg + 1) * (kFusedMaxR + 1) * p->NP;
  if (!p->om_census) return fail(SLQ_EINVAL, "the plan keeps no census (ring-fed Gram sequence created under SLQ_OMEGA=2)");
  if (len != words) return fail(SLQ_EINVAL, "census buffer: %lld words expected", (long long)words);
  HIP_TRY(hipSetDevice(p->ctx->device));
  SLQ_TRY(flush_closing_tail(p));
  HIP_TRY(hipMemcpyAsync(out, p->om_census, (size_t)words * sizeof(int), hipMemcpyDeviceToHost, p->ctx->stream));
  HIP_TRY(hipStreamSynchronize(p->ctx->stream));
  return SLQ_OK;
}

// ... its mode (0: nothing offered, 1: on, 2: verify) and, from verify runs since the last reset of the counters: out[0] the largest
// one-step innovation |measured - predicted| in units of eps_F ||A||_inf, out[1] the smallest (tol - |measured|) / rho (inf: none seen),
// out[2] the c and out[3] the kappa in use, out[4] ||A||_inf.
extern "C" int slq_plan_window_verify(slq_plan *p, int *mode, double out[5]) {
  if (!p) return fail(SLQ_EINVAL, "plan is NULL");
  if (mode) *mode = p->omega_on ? p->sw.omega : 0;
  if (!out) return SLQ_OK;
  out[0] = 0.0, out[1] = std::numeric_limits<double>::infinity(), out[2] = kOmegaC, out[3] = kOmegaKappa, out[4] = p->om_norm;
  if (!p->omega_on) return SLQ_OK;
  HIP_TRY(hipSetDevice(p->ctx->device));
  SLQ_TRY(flush_closing_tail(p));  // (asked for the numbers: `out` is null when only the mode is wanted, which flushes nothing)
  unsigned long long h[8];
  HIP_TRY(hipMemcpyAsync(h, p->om_cnt, sizeof(h), hipMemcpyDeviceToHost, p->ctx->stream));
  HIP_TRY(hipStreamSynchronize(p->ctx->stream));
  double inv;
  memcpy(&out[0], &h[kOmCntInnov], 8);
  memcpy(&inv, &h[kOmCntMargin], 8);
  if (inv > 0.0) out[1] = 1.0 / inv;
  return SLQ_OK;
}

// The same accounting for the accumulation launches of a recompute plan's replay (k_action_accumulate): ring columns read against columns offered.
extern "C" int slq_plan_action_columns(slq_plan *p, uint64_t *read, uint64_t *offered, int reset) {
  if (!p) return fail(SLQ_EINVAL, "plan is NULL");
  HIP_TRY(hipSetDevice(p->ctx->device));
  if (p->cheb_action) {
    // k_cheb_accumulate takes its mask from the host, the same for every panel: whole ring columns, counted once per launch
    if (read) *read = p->cheb_cols_read;
    if (offered) *offered = p->cheb_cols_offered;
    if (reset) p->cheb_cols_read = p->cheb_cols_offered = 0;
    HIP_TRY(hipStreamSynchronize(p->ctx->stream));
    return SLQ_OK;
  }
  unsigned long long h[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(h, p->sweep_cols_d + 2, sizeof(h), hipMemcpyDeviceToHost, p->ctx->stream));
  if (reset) HIP_TRY(hipMemsetAsync(p->sweep_cols_d + 2, 0, sizeof(h), p->ctx->stream));
  HIP_TRY(hipStreamSynchronize(p->ctx->stream));
  if (read) *read = h[0];
  if (offered) *offered = h[1];
  return SLQ_OK;
}

extern "C" int slq_plan_workspace_bytes(const slq_plan *plan, size_t *bytes) {
  if (!plan || !bytes) return fail(SLQ_EINVAL, "plan/bytes is NULL");
  *bytes = plan_workspace_bytes(plan->shape);
  return SLQ_OK;
}

// staging buffer of `cols` column-major columns
static int ensure_stage(slq_plan *p, int cols) {
  if (p->stage && p->stage_cols >= cols) return SLQ_OK;
  if (p->stage) { hipFree(p->stage); p->stage = nullptr; }
  HIP_TRY(hipMalloc(&p->stage, (size_t)cols * p->n * p->esz));
  p->stage_cols = cols;
  return SLQ_OK;
}

static int stage_chunk_cols(const slq_plan *p) {
  // ~256 MiB of staging at most
  const size_t per_col = (size_t)p->n * p->esz;
  size_t c = std::max<size_t>(1, ((size_t)256 << 20) / per_col);
  return (int)std::min<size_t>(c, (size_t)p->bpad);
}

// ||v||^2 of slot 0 -> nu_0, activity, first coefficients
// unit_entries: every entry of every probe is +-1 (Rademacher probes drawn by k_gen_probes): ||v||^2 = n is known, the norm sweep - one read of
// the panel, 0.38 ms of configs[1]'s 55 - is skipped (r04; bitwise the same nu_0: the sweep's partial sums are exact integers)
// restoring: the probes were copied back from a recompute plan's stash (replay_action) - everything else is what the original probe call did
static int init_from_probes(slq_plan *p, int sphere, bool unit_entries = false, bool restoring = false) {
  hipStream_t st = p->ctx->stream;
  if (p->basis_mode == 2 && !restoring) {
    // recompute plans: pass 2 starts from these probes again, and slq_diag_update needs v next to f(A)v
    HIP_TRY(hipMemcpyAsync(slot_ptr(p, p->v_slot), slot_ptr(p, 0), (size_t)p->slot_stride * p->esz, hipMemcpyDeviceToDevice, st));
    p->stash_unit = unit_entries;
    p->stash_ready = true;
  }
  dim3 g(p->nblkS, p->NP);
  if (!unit_entries)
    PROFILED(p, SLQ_K_AXPY_NORM,
             DISPATCH(p->dtype, p->LPR,
                      (k_axpy_norm<F, L, 1><<<g, dim3(kBlock), 0, st>>>(p->n,
                                          (F *)slot_ptr(p, 0), (const F *)nullptr,
                                          (const double *)nullptr, p->part, p->bpad))));
  PROFILED(p, SLQ_K_FINALIZE,
           hipLaunchKernelGGL(k_fin_init, dim3((p->bpad + 63) / 64), dim3(kFinThreads), 0, st, p->st, p->part,
                              unit_entries ? 0 : p->nblkS, sphere, (double)p->n));
  HIP_TRY(hipGetLastError());
  p->probes_ready = true;
  p->ran = false;
  p->cur = 0;
  p->closing.pending = false;
  return SLQ_OK;
}

// two pinned buffers of `bytes` each on the context (kept for its lifetime); false when the host cannot pin that much
static bool ensure_pinned(slq_context *ctx, size_t bytes) {
  if (ctx->pin_bytes >= bytes && ctx->pin[0] && ctx->pin[1]) return true;
  for (int b = 0; b < 2; ++b) {
    if (ctx->pin[b]) hipHostFree(ctx->pin[b]);
    ctx->pin[b] = nullptr;
    ctx->pin_busy[b] = false;
  }
  ctx->pin_bytes = 0;
  for (int b = 0; b < 2; ++b) {
    if (hipHostMalloc(&ctx->pin[b], bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (!ctx->pin_ev[b] && hipEventCreateWithFlags(&ctx->pin_ev[b], hipEventDisableTiming) != hipSuccess) return false;
  }
  ctx->pin_bytes = bytes;
  return true;
}

extern "C" int slq_plan_set_probes(slq_plan *p, const void *X, int64_t ldx) {
  if (!p || !X) return fail(SLQ_EINVAL, "plan/X is NULL");
  if (ldx < p->n) return fail(SLQ_EINVAL, "ldx (%lld) < n (%d)", (long long)ldx, p->n);
  HIP_TRY(hipSetDevice(p->ctx->device));
  hipStream_t st = p->ctx->stream;
  slq_context *ctx = p->ctx;
  // The caller's array is pageable memory: copied straight from there, the runtime bounces it through its own small
  // pinned buffers at ~10 GB/s (configs[1]: 2 GB of probes, 0.2 s). Here the columns are copied by a few host threads
  // into one of two pinned buffers (32 MiB chunks) and sent from there; the copy of chunk i + 1 overlaps the transfer
  // and the transposition kernel of chunk i. SLQ_PINNED_UPLOAD=0 keeps the direct copy.
  const size_t col_bytes = (size_t)p->n * p->esz;
  const bool pinned = p->sw.pinned_upload != 0 && (size_t)p->nprobes * col_bytes >= ((size_t)4 << 20);
  int cc = stage_chunk_cols(p);
  if (pinned) cc = (int)std::max<size_t>(1, std::min<size_t>((size_t)cc, ((size_t)32 << 20) / col_bytes));
  const bool use_pin = pinned && ensure_pinned(ctx, (size_t)cc * col_bytes);
  if (!use_pin) cc = stage_chunk_cols(p);
  SLQ_TRY(ensure_stage(p, cc));
  drop_closing_tail(p);  // (from here on ring slot 0 is written)
  // padding columns must be zero
  if (p->nprobes < p->bpad)
    HIP_TRY(hipMemsetAsync(slot_ptr(p, 0), 0, (size_t)p->slot_stride * p->esz, st));
  int buf = 0;
  for (int c0 = 0; c0 < p->nprobes; c0 += cc) {
    const int nc = std::min(cc, p->nprobes - c0);
    const char *src = (const char *)X + (size_t)c0 * (size_t)ldx * p->esz;
    if (use_pin) {
      if (ctx->pin_busy[buf]) HIP_TRY(hipEventSynchronize(ctx->pin_ev[buf]));  // its previous transfer has left the buffer
      char *dst = (char *)ctx->pin[buf];
      // rows of the chunk cut into pieces: every thread copies its row range of every column (contiguous runs)
      if (!parallel_pieces(host_threads(), p->n, [&](int, int64_t r0, int64_t r1) {
            for (int c = 0; c < nc; ++c)
              memcpy(dst + (size_t)c * col_bytes + (size_t)r0 * p->esz, src + (size_t)c * (size_t)ldx * p->esz + (size_t)r0 * p->esz, (size_t)(r1 - r0) * p->esz);
          }))
        return fail(SLQ_ENOMEM, "host worker failed while staging the probes");
      HIP_TRY(hipMemcpyAsync(p->stage, dst, (size_t)nc * col_bytes, hipMemcpyHostToDevice, st));
      HIP_TRY(hipEventRecord(ctx->pin_ev[buf], st));
      ctx->pin_busy[buf] = true;
      buf ^= 1;
    } else {
      HIP_TRY(hipMemcpy2DAsync(p->stage, col_bytes, src, (size_t)ldx * p->esz, col_bytes, (size_t)nc, hipMemcpyHostToDevice, st));
    }
    dim3 g((p->n + 63) / 64, (nc + 63) / 64);
    PROFILED(p, SLQ_K_PROBES, {
      if (p->dtype == SLQ_F64)
        hipLaunchKernelGGL(k_cols_to_panel<double>, g, dim3(256), 0, st, p->n, (const double *)p->stage, c0, nc, (double *)slot_ptr(p, 0), p->PW, p->op->perm_d.as<int32_t>());
      else
        hipLaunchKernelGGL(k_cols_to_panel<float>, g, dim3(256), 0, st, p->n, (const float *)p->stage, c0, nc, (float *)slot_ptr(p, 0), p->PW, p->op->perm_d.as<int32_t>());
    });
    if (!use_pin) HIP_TRY(hipStreamSynchronize(st));  // the caller's memory and the staging buffer are reused by the next chunk
  }
  // (pinned path: everything of X has been read when the loop ends; the device staging buffer is reused in stream order)
  p->pdf_sphere = 0;
  return init_from_probes(p, 0);
}

extern "C" int slq_plan_generate_probes(slq_plan *p, int pdf, uint64_t seed, uint64_t probe_offset) {
  if (!p) return fail(SLQ_EINVAL, "plan is NULL");
  if (pdf < 0 || pdf > 2) return fail(SLQ_EINVAL, "Invalid distribution id %d supplied.", pdf);
  HIP_TRY(hipSetDevice(p->ctx->device));
  drop_closing_tail(p);
  hipStream_t st = p->ctx->stream;
  const int RPW = 64 / p->LPR;
  const int items = (p->n + (pdf == 0 ? 127 : 1)) / (pdf == 0 ? 128 : 2);
  const int gx = std::max(1, std::min(p->ctx->num_cus * 8, (items + 4 * RPW - 1) / (4 * RPW)));
  dim3 g(gx, p->NP);
  // (an operator stored as P A P^T: the rows are scattered through the inverse permutation - the same (seed, id, row) stream)
  PROFILED(p, SLQ_K_PROBES,
           DISPATCH(p->dtype, p->LPR,
                    (k_gen_probes<F, L><<<g, dim3(256), 0, st>>>(p->n,
                                        (F *)slot_ptr(p, 0), pdf, seed, probe_offset, p->nprobes, p->op->inv_perm_d.as<int32_t>()))));
  p->pdf_sphere = (pdf == SLQ_PDF_SPHERE);
  return init_from_probes(p, p->pdf_sphere, pdf == 0 && p->sw.known_norm != 0);
}

// copy columns [c0, c0+nc) of `slot` to a host column-major array, optional per-column scale
static int panel_to_host(slq_plan *p, int slot, int c0, int nc, void *X, int64_t ldx,
                         const double *d_scale) {
  hipStream_t st = p->ctx->stream;
  const int cc = stage_chunk_cols(p);
  SLQ_TRY(ensure_stage(p, cc));
  for (int o = 0; o < nc; o += cc) {
    const int m = std::min(cc, nc - o);
    dim3 g((p->n + 63) / 64, (m + 63) / 64);
    if (p->dtype == SLQ_F64)
      hipLaunchKernelGGL(k_panel_to_cols<double>, g, dim3(256), 0, st, p->n, (const double *)slot_ptr(p, slot), c0 + o, m, (double *)p->stage, p->PW, d_scale, p->op->perm_d.as<int32_t>());
    else
      hipLaunchKernelGGL(k_panel_to_cols<float>, g, dim3(256), 0, st, p->n, (const float *)slot_ptr(p, slot), c0 + o, m, (float *)p->stage, p->PW, d_scale, p->op->perm_d.as<int32_t>());
    HIP_TRY(hipMemcpy2DAsync((char *)X + (size_t)o * (size_t)ldx * p->esz, (size_t)ldx * p->esz, p->stage,
                             (size_t)p->n * p->esz, (size_t)p->n * p->esz, (size_t)m, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  return SLQ_OK;
}

extern "C" int slq_plan_get_probes(slq_plan *p, void *X, int64_t ldx) {
  if (!p || !X) return fail(SLQ_EINVAL, "plan/X is NULL");
  if (!p->probes_ready) return fail(SLQ_EINVAL, "no probes set, or they were consumed by a run");
  if (ldx < p->n) return fail(SLQ_EINVAL, "ldx < n");
  HIP_TRY(hipSetDevice(p->ctx->device));
  return panel_to_host(p, 0, 0, p->nprobes, X, ldx, nullptr);
}


// Which kernel computes a plan's dense product (DENSE_K_*, the ids of slq_plan_dense_path): decided with the plan's shape
static int dense_kernel_of(const slq_plan *p) { return p->shape.dense_class; }

// Which kernel computes this plan's dense product, and over how many K slabs (diagnostics, tests): kernel 0 not dense, 1 k_dense_panel,
// 2 k_dense_mfma_3term, 3 k_dense_mfma_tile, 4 k_dense_mfma_lds, 5 k_dense_mfma32_lds; ksplit = dense_ks (0: no slabs). A pure function of the plan.
extern "C" int slq_plan_dense_path(slq_plan *p, int *kernel, int *ksplit) {
  if (!p) return fail(SLQ_EINVAL, "plan is NULL");
  if (kernel) *kernel = dense_kernel_of(p);
  if (ksplit) *ksplit = p->dense_ks;
  return SLQ_OK;
}

// the facts of a plan and its operator that decide what a step launches (slq_sequence.hpp)
static seq::SequenceFacts sequence_facts(const slq_plan *p) {
  seq::SequenceFacts f = p->shape.seq;
  f.nstale = p->nstale;  // (the one fact that changes under a live plan; the derived flags do not depend on it)
  return f;
}

// The layout a CSR operator would get (include/slq.h): the decision of csr_create_body - the switches read as a creation reads
// them, layout_prefilter + decide_layout - without its device half. No HIP call.
extern "C" int slq_debug_csr_layout(int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colind, int plain, int32_t *perm_out,
                                    int32_t *tile_row_out, int64_t ntile_cap, int32_t *xcd_tile_out, double *info_out) {
  if (!perm_out || !tile_row_out || !xcd_tile_out || !info_out) return fail(SLQ_EINVAL, "slq_debug_csr_layout: an output is NULL");
  return create_guarded(nullptr, [&]() {
    SLQ_TRY(validate_csr(n, nnz, rowptr, colind));
    const OperatorSwitches osw = read_operator_switches();
    const CsrView A{n, nnz, rowptr, colind};
    const OperatorLayout L = decide_layout(A, osw, layout_prefilter(A, osw, plain != 0), nullptr);
    const int64_t ntiles = L.have_tiles ? (int64_t)L.tile_row.size() - 1 : 0;
    if ((int64_t)L.tile_row.size() > ntile_cap) return fail(SLQ_EINVAL, "slq_debug_csr_layout: %zu tile boundaries, room for %lld", L.tile_row.size(), (long long)ntile_cap);
    std::copy(L.perm.begin(), L.perm.end(), perm_out);
    std::copy(L.tile_row.begin(), L.tile_row.end(), tile_row_out);
    std::copy(L.xcd_tile, L.xcd_tile + 9, xcd_tile_out);
    info_out[0] = L.have_tiles ? 1.0 : 0.0, info_out[1] = (double)ntiles, info_out[2] = L.perm.empty() ? 0.0 : 1.0, info_out[3] = L.rms_dist;
    return (int)SLQ_OK;
  });
}

// step_shape() of slq_sequence.hpp on facts given as an array (the order of seq::facts_from_array), the answer as an array (the
// order of seq::shape_to_array, then plan_sequence_of): no HIP call, so that a CPU test enumerates the decision
extern "C" int slq_debug_step_shape(const int *facts, int nfacts, int j, int prev_xt, int *out, int nout) {
  if (!facts || !out || nfacts != seq::kNumFacts || nout != seq::kNumShape + 1) return fail(SLQ_EINVAL, "slq_debug_step_shape: %d facts in, %d values out", seq::kNumFacts, seq::kNumShape + 1);
  const seq::SequenceFacts f = seq::facts_from_array(facts);
  seq::shape_to_array(seq::step_shape(f, j, prev_xt != 0), out);
  out[seq::kNumShape] = seq::plan_sequence_of(f);
  return SLQ_OK;
}

// dense operator on MFMA (fp64, and fp32 through k_dense_mfma32_lds): Wn = sc*(A Wc) - cp*Wp with alpha partials (plain = 0), or Wn = A Wc
static int launch_dense_mfma(slq_plan *p, const void *Wc, const void *Wp, void *Wn, int first, int plain, int *nblk_out) {
  const slq_operator *op = p->op;
  hipStream_t st = p->ctx->stream;
  // panels of 32+ columns: big tiles, K split over workgroups, epilogue by k_3term_slabs (k_dense_mfma_tile);
  // 16-column panels: the 16-row kernel with its fused epilogue. SLQ_DENSE_TILE16=1 forces the latter (A/B runs).
  const int kernel = dense_kernel_of(p);
  if (kernel == DENSE_K_LDS32) {
    const int ks = p->dense_ks;
    float *raw = (float *)p->T + p->slot_stride;  // slabs 1..ks of T (slab 0 is the unfused product)
    const dim3 g((p->n + kDense32BM - 1) / kDense32BM, p->NP, ks);
    const int a_vec = op->lda % 4 == 0 && ((uintptr_t)op->csr.vals.p & 15) == 0;
    for (int col0 = 0; col0 < p->PW; col0 += kDense32BN)  // PW = 128 / 256: A streamed once per 64 columns (32 flop per byte of A: still MFMA-bound)
      k_dense_mfma32_lds<<<g, dim3(kBlock), 0, st>>>(p->n, op->csr.vals.as<const float>(), op->lda, a_vec, (const float *)Wc, p->PW, col0, raw, p->slot_stride);
    const dim3 gS(p->nblkS, p->NP);
    DISPATCH(SLQ_F32, p->LPR,
             (k_3term_slabs<F, L><<<gS, dim3(kBlock), 0, st>>>(p->n, (const F *)raw, ks, p->slot_stride, (const F *)Wc, (const F *)Wp, (F *)Wn,
                                                             p->st.coefA, p->part, p->bpad, first, plain)));
    if (nblk_out) *nblk_out = p->nblkS;
    return SLQ_OK;
  }
  if (kernel == DENSE_K_LDS || kernel == DENSE_K_TILE) {
    const int ks = p->dense_ks;
    double *raw = (double *)p->T + p->slot_stride;  // slabs 1..ks of T (slab 0 is the unfused product)
    const int ncg = p->PW >= 64 ? 2 : 1;
    const int rw = 32 * (kWaves / ncg);
    const dim3 g((p->n + rw - 1) / rw, p->NP, ks);
    for (int col0 = 0; col0 < p->PW; col0 += 32 * ncg) {  // PW = 128: two 64-column halves, A streamed twice
      if (kernel == DENSE_K_LDS)
        k_dense_mfma_lds<2><<<g, dim3(kBlock), 0, st>>>(p->n, op->csr.vals.as<const double>(), op->lda, (const double *)Wc, p->PW, col0, raw, p->slot_stride);
      else if (ncg == 2)
        k_dense_mfma_tile<2><<<g, dim3(kBlock), 0, st>>>(p->n, op->csr.vals.as<const double>(), op->lda, (const double *)Wc, p->PW, col0, raw, p->slot_stride);
      else
        k_dense_mfma_tile<1><<<g, dim3(kBlock), 0, st>>>(p->n, op->csr.vals.as<const double>(), op->lda, (const double *)Wc, p->PW, col0, raw, p->slot_stride);
    }
    // second stage: sum the slabs in slab order, three-term epilogue and alpha partials (or the plain product)
    const dim3 gS(p->nblkS, p->NP);
    DISPATCH(SLQ_F64, p->LPR,
             (k_3term_slabs<F, L><<<gS, dim3(kBlock), 0, st>>>(p->n, (const F *)raw, ks, p->slot_stride, (const F *)Wc, (const F *)Wp, (F *)Wn,
                                                             p->st.coefA, p->part, p->bpad, first, plain)));
    if (nblk_out) *nblk_out = p->nblkS;
    return SLQ_OK;
  }
  const size_t part_rows = (size_t)kReorthChunk * p->part_maxblk;
  const int nblk = (p->n + 15) / 16;
  if ((size_t)nblk > part_rows) return fail(SLQ_EINVAL, "dense operator too large for the partials buffer");
  const dim3 g(nblk, p->NP);
#define DENSE_LAUNCH(TWV, COL0)                                                                             \
  {                                                                                                         \
    const size_t lds = ((size_t)kWaves * (TWV / 16) * 4 * 64 + (size_t)TWV * 4) * sizeof(double);          \
    k_dense_mfma_3term<TWV><<<g, dim3(kBlock), lds, st>>>(p->n, op->csr.vals.as<const double>(), op->lda, (const double *)Wc,        \
                                                        (const double *)Wp, (double *)Wn, p->st.coefA, p->part, p->bpad, first, plain, p->PW, COL0); \
  }
  switch (p->PW) {
    case 128: DENSE_LAUNCH(64, 0) DENSE_LAUNCH(64, 64) break;
    case 64: DENSE_LAUNCH(64, 0) break;
    case 32: DENSE_LAUNCH(32, 0) break;
    default: DENSE_LAUNCH(16, 0) break;
  }
#undef DENSE_LAUNCH
  if (nblk_out) *nblk_out = nblk;
  return SLQ_OK;
}

// A preconditioned kernel operator whose base has new hyperparameters is stale until slq_kernel_precond_refresh: its factor, G and
// logdet P belong to the old ones. Every product, apply and plan run asks here first (a captured graph is not replayed either).
static int precond_check_fresh(const slq_operator *op, const char *who) {
  if (op->kind == OP_KERNEL_PRECOND) SLQ_TRY(kernel_refuse_scaled(op->pre->base, who));  // (a base scaled after the factor was built: DESIGN.md §4.23)
  if (op->kind != OP_KERNEL_PRECOND || op->pre->epoch == op->pre->base->k_epoch) return SLQ_OK;
  return fail(SLQ_EINVAL, "%s: the preconditioner is stale: call slq_kernel_precond_refresh (the base operator's hyperparameters have changed)", who);
}

// kernel operator: T = A W_c by k_kernel_panel (slq_kernelop.hpp). One slab: straight into T; a j split (small n): slab z into
// T + (1 + z) slots, summed in slab order into T by k_3term_slabs (plain) - the slabs the plan's shape allocated (dense_ks)
// op: the operator whose points are read (the plan's own, or the base of a preconditioned one)
static int launch_kernel_product(slq_plan *p, const slq_operator *op, const void *Wc) {
  hipStream_t st = p->ctx->stream;
  const KernelSchedule S = kernel_schedule(p->n, p->PW, p->NP, p->ctx->num_cus);
  if ((S.nslabs > 1 ? S.nslabs : 0) != p->dense_ks) return fail(SLQ_EINVAL, "kernel operator: the plan holds %d slabs, the schedule asks for %d", p->dense_ks, S.nslabs);
  int log2pw = 0;
  while ((1 << log2pw) < p->PW) ++log2pw;
  char *raw = (char *)p->T + (S.nslabs > 1 ? (size_t)p->slot_stride * p->esz : 0);
  const KernelPanelArgs a{p->n, (int)op->k_pts.npad, op->k_pts.dpad / 4, op->k_pts.zt, op->k_pts.nrm, op->k_pts.params, Wc, log2pw, p->NP * p->PW, raw, p->slot_stride,
                          op->k_scaled ? op->k_c.p : nullptr};
  // (a diagonal scale, DESIGN.md §4.23: another kernel, the same schedule and slab sum - which is why the scale is in the graph key, graph_variant)
  bool ok;
  if (op->k_scaled) ok = p->dtype == SLQ_F64 ? kernel_panel_scaled_launch<double>(op->k_profile, S, a, st) : kernel_panel_scaled_launch<float>(op->k_profile, S, a, st);
  else ok = p->dtype == SLQ_F64 ? kernel_panel_launch<double>(op->k_profile, S, a, st) : kernel_panel_launch<float>(op->k_profile, S, a, st);
  if (!ok) return fail(SLQ_EINVAL, "kernel operator: no product kernel for profile %d with %d column tiles", op->k_profile, S.col_blocks);
  if (S.nslabs > 1) {
    const dim3 gS(p->nblkS, p->NP);
    DISPATCH(p->dtype, p->LPR,
             (k_3term_slabs<F, L><<<gS, dim3(kBlock), 0, st>>>(p->n, (const F *)raw, S.nslabs, p->slot_stride, (const F *)Wc, (const F *)nullptr, (F *)p->T,
                                                             p->st.coefA, p->part, p->bpad, 1, 1)));
  }
  HIP_TRY(hipGetLastError());
  return SLQ_OK;
}

// Toeplitz operator: T = A W_c by FFT passes along the rows of the panel as it stands (slq_toeplitz.hip): panel after panel through the
// plan's one complex workspace (WS_T2), one to five launches each. Every address is fixed: a captured graph replays it.
static int launch_toeplitz_product(slq_plan *p, const slq_operator *op, const char *Wc) {
  const ToeplitzPlan P = toeplitz_plan(p->n, (int)p->esz, p->PW);
  if (P.ws_bytes != p->shape.ws[WS_T2].bytes) return fail(SLQ_EINVAL, "Toeplitz operator: the plan holds %zu workspace bytes, the product asks for %zu", p->shape.ws[WS_T2].bytes, P.ws_bytes);
  const size_t panel_bytes = (size_t)p->n * p->PW * p->esz;
  for (int pnl = 0; pnl < p->NP; ++pnl) {
    ToeplitzLaunch a;
    a.W = Wc + (size_t)pnl * panel_bytes;
    a.T = (char *)p->T + (size_t)pnl * panel_bytes;
    a.ws = p->T2;
    a.sym = op->tz_sym.p, a.tab = op->tz_tab.p, a.tw[0] = op->tz_tw[0].p, a.tw[1] = op->tz_tw[1].p;
    a.pw = p->PW, a.col0 = pnl * p->PW, a.nprobes = p->nprobes;
    const int rc = toeplitz_launch(p->dtype == SLQ_F64, P, a, p->ctx->stream);
    if (rc == kToeplitzBadGeometry) return fail(SLQ_EINVAL, "Toeplitz product: a panel of %d columns is no multiple of the %d a workgroup owns", p->PW, 2 * P.cg);
    if (rc != 0) return fail(SLQ_EHIP, "Toeplitz product: %s", hipGetErrorString((hipError_t)rc));
  }
  return SLQ_OK;
}

// T = A * (slot c), unscaled, for operators without a fused kernel
static int apply_operator_unfused(slq_plan *p, int slot_c) {
  hipStream_t st = p->ctx->stream;
  slq_operator *op = p->op;
  if (op->kind == OP_KERNEL) {
    PROFILED(p, SLQ_K_SPMM, SLQ_TRY(launch_kernel_product(p, op, slot_ptr(p, slot_c))));
    return SLQ_OK;
  }
  if (op->kind == OP_TOEPLITZ) {
    PROFILED(p, SLQ_K_SPMM, SLQ_TRY(launch_toeplitz_product(p, op, slot_ptr(p, slot_c))));
    return SLQ_OK;
  }
  if (op->kind == OP_KERNEL_PRECOND) {
    // T = M A M W_c: V = M W_c, T = A V by the base's product, T = M T in place (slq_kernelprecond.hpp). V, the slab partials
    // and G L^T W are the plan's own scratch (WS_T2): a captured graph holds their addresses.
    SLQ_TRY(precond_check_fresh(op, "plan"));
    const KernelPrecond &pc = *op->pre;
    double *V = (double *)p->T2, *scratch = V + p->slot_stride;
    const int cols = p->NP * p->PW;
    const PrecondPanelLayout lay{p->n, p->PW};
    const auto apply = [&](const double *X, double *Y) {
      return precond_apply_launch(p->n, pc.L.as<const double>(), pc.rpad, pc.G.as<const double>(), (const double *)pc.base->k_pts.params, X, Y, cols, lay, scratch,
                                  p->ctx->num_cus, st);
    };
    PROFILED(p, SLQ_K_SPMM, {
      if (!apply((const double *)slot_ptr(p, slot_c), V)) return fail(SLQ_EINVAL, "preconditioned kernel operator: no apply kernel for rank %d", pc.rpad);
    });
    PROFILED(p, SLQ_K_SPMM, SLQ_TRY(launch_kernel_product(p, pc.base, V)));
    PROFILED(p, SLQ_K_SPMM, {
      if (!apply((const double *)p->T, (double *)p->T)) return fail(SLQ_EINVAL, "preconditioned kernel operator: no apply kernel for rank %d", pc.rpad);
    });
    HIP_TRY(hipGetLastError());
    return SLQ_OK;
  }
  if (dense_kernel_of(p) >= DENSE_K_3TERM) {
    PROFILED(p, SLQ_K_SPMM, SLQ_TRY(launch_dense_mfma(p, slot_ptr(p, slot_c), nullptr, p->T, 1, 1, nullptr)));
    return SLQ_OK;
  }
  if (op->kind == OP_DENSE) {
    dim3 g(std::max(1, std::min(p->ctx->num_cus * 2, (p->n + kWaves - 1) / kWaves)), p->NP);
    PROFILED(p, SLQ_K_SPMM,
             DISPATCH(p->dtype, p->LPR,
                      (k_dense_panel<F, L><<<g, dim3(kBlock), 0, st>>>(p->n,
                                          (op->dense_t ? op->dense_t : op->csr.vals).as<const F>(), op->lda, (const F *)slot_ptr(p, slot_c), (F *)p->T))));
    return SLQ_OK;
  }
  if (op->kind == OP_GRAM) {
    // T = A^T (A W_c): two plain panel SpMMs through an mrows-row panel (eigen_operators.h:66-72, gram = true)
    const dim3 g1(std::max(1, std::min(p->nblkS, (int)((op->mrows + kWaves - 1) / kWaves))), p->NP), g2(p->nblkS, p->NP);
    PROFILED(p, SLQ_K_SPMM,
             DISPATCH(p->dtype, p->LPR,
                      (k_spmm_plain<F, L><<<g1, dim3(kBlock), 0, st>>>((int)op->mrows, op->csr.rp(), op->csr.ci(), op->csr.vals.as<const F>(),
                                                                   (const F *)slot_ptr(p, slot_c), (F *)p->T2, p->n))));
    PROFILED(p, SLQ_K_SPMM,
             DISPATCH(p->dtype, p->LPR,
                      (k_spmm_plain<F, L><<<g2, dim3(kBlock), 0, st>>>(p->n, op->transposed.rp(), op->transposed.ci(), op->transposed.vals.as<const F>(),
                                                                   (const F *)p->T2, (F *)p->T, (int)op->mrows))));
    return SLQ_OK;
  }
  if (op->kind == OP_DEVICE_CALLBACK) {
    // device plugin: the panel goes through two column-major staging buffers in HBM (X | Y); the plugin
    // enqueues Y = A X on our stream (or synchronises itself) - nothing crosses PCIe
    const int cc = std::max(1, stage_chunk_cols(p) / 2);
    SLQ_TRY(ensure_stage(p, 2 * cc));
    char *sx = (char *)p->stage, *sy = sx + (size_t)cc * p->n * p->esz;
    HIP_TRY(hipMemsetAsync(p->T, 0, (size_t)p->slot_stride * p->esz, st));
    for (int c0 = 0; c0 < p->nprobes; c0 += cc) {
      const int nc = std::min(cc, p->nprobes - c0);
      dim3 g((p->n + 63) / 64, (nc + 63) / 64);
      if (p->dtype == SLQ_F64)
        hipLaunchKernelGGL(k_panel_to_cols<double>, g, dim3(256), 0, st, p->n, (const double *)slot_ptr(p, slot_c), c0, nc, (double *)sx, p->PW, (const double *)nullptr, (const int32_t *)nullptr);
      else
        hipLaunchKernelGGL(k_panel_to_cols<float>, g, dim3(256), 0, st, p->n, (const float *)slot_ptr(p, slot_c), c0, nc, (float *)sx, p->PW, (const double *)nullptr, (const int32_t *)nullptr);
      if (op->dev_fn(op->user, sx, sy, p->n, nc, (void *)st) != 0)
        return fail(SLQ_ECALLBACK, "device operator callback failed on columns %d..%d", c0, c0 + nc - 1);
      if (p->dtype == SLQ_F64)
        hipLaunchKernelGGL(k_cols_to_panel<double>, g, dim3(256), 0, st, p->n, (const double *)sy, c0, nc, (double *)p->T, p->PW, (const int32_t *)nullptr);
      else
        hipLaunchKernelGGL(k_cols_to_panel<float>, g, dim3(256), 0, st, p->n, (const float *)sy, c0, nc, (float *)p->T, p->PW, (const int32_t *)nullptr);
      HIP_TRY(hipGetLastError());
    }
    return SLQ_OK;
  }
  // host callback: device -> host, one matvec per probe, host -> device
  const size_t colb = (size_t)p->n * p->esz;
  if (p->hbuf.size() < 2 * colb * (size_t)p->nprobes) p->hbuf.resize(2 * colb * (size_t)p->nprobes);
  char *hx = p->hbuf.data(), *hy = hx + colb * p->nprobes;
  SLQ_TRY(panel_to_host(p, slot_c, 0, p->nprobes, hx, p->n, nullptr));
  for (int i = 0; i < p->nprobes; ++i)
    if (op->fn(op->user, hx + colb * i, hy + colb * i) != 0)
      return fail(SLQ_ECALLBACK, "operator callback failed on probe %d", i);
  const int cc = stage_chunk_cols(p);
  HIP_TRY(hipMemsetAsync(p->T, 0, (size_t)p->slot_stride * p->esz, st));
  for (int c0 = 0; c0 < p->nprobes; c0 += cc) {
    const int nc = std::min(cc, p->nprobes - c0);
    HIP_TRY(hipMemcpyAsync(p->stage, hy + colb * c0, colb * nc, hipMemcpyHostToDevice, st));
    dim3 g((p->n + 63) / 64, (nc + 63) / 64);
    if (p->dtype == SLQ_F64)
      hipLaunchKernelGGL(k_cols_to_panel<double>, g, dim3(256), 0, st, p->n, (const double *)p->stage, c0, nc, (double *)p->T, p->PW, p->op->perm_d.as<int32_t>());
    else
      hipLaunchKernelGGL(k_cols_to_panel<float>, g, dim3(256), 0, st, p->n, (const float *)p->stage, c0, nc, (float *)p->T, p->PW, p->op->perm_d.as<int32_t>());
    HIP_TRY(hipStreamSynchronize(st));
  }
  return SLQ_OK;
}

static int launch_reorth_update(slq_plan *p, int j, int r, int istart, bool axpy = false, int klass = SLQ_K_REORTH_UPD);
static int launch_reorth_update_range(slq_plan *p, int j, int ibegin, int iend, bool axpy = false, int klass = SLQ_K_REORTH_UPD);
static int update_chunk_cols(const slq_plan *p);

// probes per workgroup of the QL kernel: 3*deg*lanes doubles of LDS, at most 150 KiB
static int quadrature_lanes(int deg) {
  int lanes = (int)((150 * 1024) / ((size_t)3 * deg * 8));
  return std::max(1, std::min(64, lanes));
}
// the launch of k_quadrature: deg <= 64 runs one probe per wave with the Jacobi matrix across the lanes (lanes = 0, no LDS,
// a workgroup per probe); a longer matrix runs one probe per lane out of LDS
struct QuadShape {
  int lanes;
  unsigned grid;
  size_t lds;
};
static QuadShape quadrature_shape(int deg, int nprobes) {
#ifndef SLQ_AB_QL_LDS  // (A/B build: the LDS form at every degree)
  if (deg <= 64) return {0, (unsigned)nprobes, 0};
#endif
  const int lanes = quadrature_lanes(deg);
  return {lanes, (unsigned)((nprobes + lanes - 1) / lanes), (size_t)3 * deg * lanes * 8};
}

// the generic update pass of the Gram sequence (k_csr_pass<PASS_UPDATEG>, nontemporal streams), r = 1 .. kFusedMaxR ring columns
template <typename F, int L, int RC> static inline void launch_csr_updateg_rc(slq_plan *p, bool pipe_on, dim3 grid, size_t lds, hipStream_t st, int j, int xt);
template <typename F, int L> static inline void launch_csr_updateg(slq_plan *p, int r, bool pipe_on, dim3 grid, size_t lds, hipStream_t st, int j, int xt) {
  switch (r) {
    case 1: launch_csr_updateg_rc<F, L, 1>(p, pipe_on, grid, lds, st, j, xt); break;
    case 2: launch_csr_updateg_rc<F, L, 2>(p, pipe_on, grid, lds, st, j, xt); break;
    case 3: launch_csr_updateg_rc<F, L, 3>(p, pipe_on, grid, lds, st, j, xt); break;
    case 4: launch_csr_updateg_rc<F, L, 4>(p, pipe_on, grid, lds, st, j, xt); break;
    case 5: launch_csr_updateg_rc<F, L, 5>(p, pipe_on, grid, lds, st, j, xt); break;
    case 6: launch_csr_updateg_rc<F, L, 6>(p, pipe_on, grid, lds, st, j, xt); break;
    case 7: launch_csr_updateg_rc<F, L, 7>(p, pipe_on, grid, lds, st, j, xt); break;
    default: launch_csr_updateg_rc<F, L, 8>(p, pipe_on, grid, lds, st, j, xt); break;
  }
}

// one dots sweep of the store-and-revisit sequence (deferred: the block-CGS sweeps leave `w -= cB W_c` to the update sweep -
// every dots chunk applies it in registers and stores nothing)
template <typename F, int L> static inline void launch_reorth_dot(slq_plan *p, dim3 gS, hipStream_t st, int j, int i0, int rc) {
  k_reorth_dot<F, L><<<gS, dim3(kBlock), 0, st>>>(p->n, (F *)p->ring, p->slot_stride, p->S, j, i0, rc, p->sw.defer_axpy ? 2 : (int)(i0 == 0), p->st.coefB, p->part,
                                                  p->bpad);
}
template <typename F, int L>
static inline void launch_reorth_update_kernel(slq_plan *p, dim3 gS, size_t lds, hipStream_t st, int j, int i0, int rc, bool axpy = false) {
  k_reorth_update<F, L><<<gS, dim3(kBlock), lds, st>>>(p->n, (F *)p->ring, p->slot_stride, p->S, j, i0, rc, p->st.gamma + (size_t)i0 * p->bpad,
                                                     p->part, p->bpad, axpy ? p->st.coefB : nullptr, p->sweep_cols_d, p->sweep_skip ? 1 : 0);
}

// one fused CSR pass; the pipelined row loop exists for one-row-per-wave panels (L == 64) and not for the alpha pass
template <typename F, int L, int PASS, int LP, int RC, typename... Args>
static inline void launch_csr_pass(bool pipe_on, dim3 grid, size_t lds, hipStream_t st, Args... args) {
  if constexpr (L == 64 && PASS != PASS_ALPHA) {
    if (pipe_on) {
      k_csr_pass<F, L, PASS, LP, RC, 1><<<grid, dim3(kBlock), lds, st>>>(args...);
      return;
    }
  }
  k_csr_pass<F, L, PASS, LP, RC, 0><<<grid, dim3(kBlock), lds, st>>>(args...);
}

template <typename F, int L, int RC> static inline void launch_csr_updateg_rc(slq_plan *p, bool pipe_on, dim3 grid, size_t lds, hipStream_t st, int j, int xt) {
  const slq_operator *op = p->op;
  launch_csr_pass<F, L, PASS_UPDATEG, 1, RC>(pipe_on, grid, lds, st, p->n, op->csr.rp(), op->csr.ci(), op->csr.vals.as<const F>(), (F *)p->ring, p->slot_stride, p->S, j, p->st.coefA,
                                             p->st.coefB, p->st.gamma, p->part, p->bpad, xt);
}

// the same pass on workgroup tiles (wide panels only; slq_kernels.hpp: k_csr_tile_pass). xt is the kernel's complete word
// (step_shape); upper: the alpha-only pass reads the upper-triangle stream
template <typename F, int L, int PASS, int LP, int RC>
static inline void launch_tile_pass(slq_plan *p, dim3 grid, size_t lds, hipStream_t st, int j, int xt, bool upper) {
  if constexpr (L == 64 && (PASS == PASS_ALPHA || PASS == PASS_ADOTS || PASS == PASS_UPDATE || PASS == PASS_SPMM)) {
    const slq_operator *op = p->op;
    TileRanges xr;
    for (int x = 0; x < 9; ++x) xr.first[x] = op->tiles.xcd_tile[x];
    if constexpr (RC <= kRingMaxR) {
      if (op->tiles_ringed) {
        // the ring-fed variant: flag words and descriptor staging + kRingSlots slots; 16 waves per workgroup
        const size_t lds_ring = kRingHeadBytes + (size_t)kRingSlots * (kRingTileCols * 1024 + kRingMetaBytes);
        // (the base tiles' full stream whatever stream the plan's other passes read; the upper one is the plan's)
        const TileStream *ts = upper ? p->rs_upper : &op->streams[0].full;
        if (!ts) {
          p->launch_error = true;
          return;
        }
        if (upper)
          for (int x = 0; x < 9; ++x) xr.first[x] = p->shape.rs_xcd_u[x];
        k_csr_ring_pass<F, PASS, LP, RC><<<grid, dim3(kRingBlock), lds_ring, st>>>(p->n, ts->desc.as<int32_t>(), ts->rec.as<char>(), xr, (F *)p->ring, p->slot_stride, p->S, j, p->st.coefA,
                                                                               p->st.coefB, p->st.gamma, p->part, p->bpad, xt, p->ring_fail_d);
        return;
      }
    }
    if (op->tiles_ringed) {  // never reached (step_shape sends ring-sized tiles to the ring-fed kernels or the generic passes)
      p->launch_error = true;  // (no launch: enqueue_run turns this into SLQ_EINVAL instead of handing out numbers of a pass that never ran)
      return;
    }
    if constexpr (PASS != PASS_SPMM)
    k_csr_tile_pass<F, PASS, LP, RC><<<grid, dim3(kBlock), lds, st>>>(p->n, op->csr.rp(), op->csr.vals.as<const F>(), op->tiles.tile_row.as<int32_t>(), op->tiles.tile_ptr.as<int32_t>(),
                                                                    op->tiles.tile_cols.as<int32_t>(), op->tiles.lcol.as<int32_t>(), op->tiles.self_idx.as<int32_t>(), xr, op->tiles.max_cols, (F *)p->ring,
                                                                    p->slot_stride, p->S, j, p->st.coefA, p->st.coefB, p->st.gamma, p->part, p->bpad, xt);
  }
}

#ifdef SLQ_DEBUG_TIMES
static unsigned long long *g_dbg_host_handle = nullptr;
static unsigned long long *debug_times_buffer() { return g_dbg_host_handle; }
#else
static unsigned long long *debug_times_buffer() { return nullptr; }
#endif

// one ring-fed pass through k_ring_pass (slq_ring.hpp: any panel width, up to 8 ring columns; nontemporal streams). xt is the
// kernel's complete word (step_shape); upper: the alpha-only pass reads the upper-triangle stream
static int launch_ring_gen(slq_plan *p, int pass, int rc, dim3 grid, hipStream_t st, int j, int xt, bool upper, const int *wread = nullptr) {
  RingArgs a;
  a.pass = pass;
  a.rc = rc;
  a.staged = (pass == PASS_ALPHA && p->ring_staged) ? 1 : 0;
  a.grid = grid;
  a.st = st;
  a.n = p->n;
  const TileStream *ts = upper ? p->rs_upper : p->rs_full;
  if (!ts) return fail(SLQ_EINVAL, "a ring-fed pass without its tile stream");
  a.desc = ts->desc.as<int32_t>();
  a.rec = ts->rec.as<char>();
  for (int x = 0; x < 9; ++x) a.xr.first[x] = upper ? p->shape.rs_xcd_u[x] : p->shape.rs_xcd[x];
  a.ring = p->ring;
  a.slot_stride = p->slot_stride;
  a.S = p->S;
  a.j = j;
  a.coefA = p->st.coefA;
  a.coefB = p->st.coefB;
  a.gamma = p->st.gamma;
  a.part = p->part;
  a.bpad = p->bpad;
  a.xt = xt;
  a.fail = p->ring_fail_d;
  a.wread = wread;
  a.dbg = pass == p->sw.debug_pass ? debug_times_buffer() : nullptr;  // (diagnostic builds: the pass whose time line is stamped)
  const bool d = p->dtype == SLQ_F64;
  int rc_l = -1;
  switch (p->LPR) {
    case 64: rc_l = d ? slq_ring_launch_f64_l64(a) : slq_ring_launch_f32_l64(a); break;
    case 32: rc_l = d ? slq_ring_launch_f64_l32(a) : slq_ring_launch_f32_l32(a); break;
    case 16: rc_l = d ? slq_ring_launch_f64_l16(a) : slq_ring_launch_f32_l16(a); break;
    default: break;
  }
  if (rc_l != 0) return fail(SLQ_EINVAL, "no ring-fed kernel for pass %d with %d ring columns on %d lanes per row", pass, rc, p->LPR);
  return SLQ_OK;
}

// what the launches of one enqueue_run share: grids, tolerances, the LDS sizes of the fused passes
struct RunFrame {
  slq_plan *p;
  hipStream_t st;
  bool nt;
  double eps, residual_tol, orth_tol;
  dim3 gA, gS, gU, gF, gAf, gT;
  size_t lds0;  // the fused passes' static part
  OmegaState om_off;
  int blocks(int blk) const {
    switch (blk) {
      case seq::BLK_A: return p->nblkA;
      case seq::BLK_U: return p->nblkU;
      case seq::BLK_T: return p->nblkT;
      case seq::BLK_F: return p->nblkF;
      default: return p->nblkS;
    }
  }
  // alpha pass: grid and residency cap (nblkF, alpha_pad) are chosen in slq_plan_create
  size_t lds_alpha(const seq::StepShape &s) const { return lds0 + (s.alpha_tiled ? 0 : p->alpha_pad); }
  // dots/update passes: 64 KiB of LDS padding pins residency at 2 workgroups per CU whatever the variant's
  // register count (62-96 VGPRs would admit 3 for some). Their grid is 2 per CU *per panel*: blocks are
  // dispatched panel-major, so panel 0 fills the chip, panel 1 follows as its workgroups retire, and an
  // XCD's L2 holds one panel's gather halo at a time (both panels side by side fetch 9.2/10.8 GB per
  // dots/update launch instead of 6.5/8.6 GB).
  // (the pipelined row loop runs ONE resident workgroup per CU: 96 KiB of padding)
  size_t lds_fused(const seq::StepShape &s) const {
    return lds0 + (s.tiled ? 0 : (size_t)(p->sw.fused_pad >= 0 ? p->sw.fused_pad : (p->pipelined ? 98304 : 65536)));
  }
  // wide panels (one row per wave) of an operator with barrier tiles: the tile's distinct panel rows are staged once in LDS
  size_t lds_tile(const seq::StepShape &s) const {
    return lds0 + (s.tiled ? (size_t)(SLQ_TILE_DB ? 2 : 1) * p->op->tiles.max_cols * p->PW * p->esz : 0);
  }
};

// one fused pass of step j as the shape says: k_ring_pass, the tile kernels or the generic k_csr_pass (the macros are the
// template dispatch over PASS, load policy and ring columns, nothing else)
#define CSR_PASS_RC(PASS, LP, RCT)                                                                   \
  do {                                                                                               \
    if (tl && s.gen)                                                                                 \
      SLQ_TRY(launch_ring_gen(p, PASS, RCT, c.gT, c.st, j, xt, upper));                              \
    else if (tl)                                                                                     \
      DISPATCH(p->dtype, p->LPR, (launch_tile_pass<F, L, PASS, LP, RCT>(p, c.gT, c.lds_tile(s), c.st, j, xt, upper))); \
    else                                                                                             \
      DISPATCH(p->dtype, p->LPR,                                                                     \
               (launch_csr_pass<F, L, PASS, LP, RCT>(s.pipe_on != 0, (PASS == PASS_ALPHA ? c.gAf : c.gU), lds, c.st, p->n, \
                   (half ? op->upper : op->csr).rp(), (half ? op->upper : op->csr).ci(),               \
                   (half ? op->upper : op->csr).vals.as<const F>(), (F *)p->ring, p->slot_stride, p->S, j, \
                   p->st.coefA, p->st.coefB, p->st.gamma, p->part, p->bpad, xt)));                   \
  } while (0)
#define CSR_PASS(PASS, LP)                                                                           \
  switch (PASS == PASS_ALPHA ? 0 : rc) {                                                             \
    case 0: CSR_PASS_RC(PASS, LP, ((PASS == PASS_DOTS || PASS == PASS_ADOTS) ? 1 : 0)); break;       \
    case 1: CSR_PASS_RC(PASS, LP, (PASS == PASS_ALPHA ? 0 : 1)); break;                              \
    case 2: CSR_PASS_RC(PASS, LP, (PASS == PASS_ALPHA ? 0 : 2)); break;                              \
    case 3: CSR_PASS_RC(PASS, LP, (PASS == PASS_ALPHA ? 0 : 3)); break;                              \
    case 4: CSR_PASS_RC(PASS, LP, (PASS == PASS_ALPHA ? 0 : 4)); break;                              \
    case 5: CSR_PASS_RC(PASS, LP, (PASS == PASS_ALPHA ? 0 : 5)); break;                              \
    case 6: CSR_PASS_RC(PASS, LP, (PASS == PASS_ALPHA ? 0 : 6)); break;                              \
    case 7: CSR_PASS_RC(PASS, LP, (PASS == PASS_ALPHA ? 0 : 7)); break;                              \
    default: CSR_PASS_RC(PASS, LP, (PASS == PASS_ALPHA ? 0 : 8)); break;                             \
  }
template <int PASS> static int launch_fused_pass(const RunFrame &c, const seq::StepShape &s, int j, int rc, size_t lds, int xt) {
  slq_plan *p = c.p;
  const slq_operator *op = p->op;
  const bool tl = PASS == PASS_ALPHA ? s.alpha_tiled : s.tiled;
  const bool half = PASS == PASS_ALPHA && s.half;
  const bool upper = PASS == PASS_ALPHA && s.alpha_upper;
  if (c.nt) CSR_PASS(PASS, 1) else CSR_PASS(PASS, 0)
  return SLQ_OK;
}
#undef CSR_PASS
#undef CSR_PASS_RC

// Gram sequence on ring-fed plans (r >= 1): alpha-only pass, projections from the Gram rows of the last two update passes
// (k_fin_gram), update pass that also takes the new vector against every ring column it reads (slq_kernels.hpp)
// part (here and in the three launchers below): the whole step, or what stands in front of its update pass / the update pass
// and the scalar kernel behind it alone (seq::StepPart: the closing tail of a run)
static int launch_gram_ring(const RunFrame &c, const seq::StepShape &s, int j, int part) {
  slq_plan *p = c.p;
  hipStream_t st = c.st;
  const int bp = p->bpad, r = s.r, S = p->S;
  if (part & seq::STEP_FRONT) PROFILED(p, SLQ_K_SPMM, SLQ_TRY(launch_fused_pass<PASS_ALPHA>(c, s, j, 0, c.lds_alpha(s), s.xt_alpha)));
  // a full window of three columns is offered to the edge recurrence (slq_kernels.hpp: OmegaState): its oldest column is read only
  // where the panel's flag says so. The launch sequence does not depend on the flags: the rescue kernel is always there.
  OmegaState om = c.om_off;
  om.census = p->om_census, om.PW = p->PW, om.NP = p->NP;
  if (s.omega) {
    om.mode = p->sw.omega;
    om.est_prev = s.est_prev;
    om.force = (j == p->sw.omega_trip ? 1 : 0) | (j == p->sw.omega_rescue ? 2 : 0);
    om.D = p->om_buf, om.rho = p->om_buf + bp, om.g3 = p->om_buf + 2 * (size_t)bp, om.Dm = p->om_buf + 3 * (size_t)bp;
    om.read = p->om_flags, om.rescue = p->om_flags + (size_t)(p->deg + 1) * p->NP;
    om.cnt = p->om_cnt;
    om.eps_norm = c.eps * p->om_norm;
    om.theta = kOmegaC * om.eps_norm;
    om.tol_k = c.orth_tol / kOmegaKappa;
  }
  if (part & seq::STEP_FRONT)
    PROFILED(p, SLQ_K_FINALIZE,
             hipLaunchKernelGGL(k_fin_gram, dim3((bp + 63) / 64, r), dim3(kFinThreads), 0, st, p->st, p->part, c.blocks(s.blk_alpha), j, r, c.orth_tol, om, (int)(part == seq::STEP_FRONT)));
  if ((part & seq::STEP_FRONT) && om.mode == 1 && om.est_prev) {
    double *part_r = p->part + (size_t)p->part_maxblk * bp;  // (behind the alpha partials, which the second pass does not need but the slab layout keeps)
    // (one launch: the workgroup that finishes a flagged panel last sums its partials and takes the edge position again)
    PROFILED(p, SLQ_K_FINALIZE,
             DISPATCH(p->dtype, p->LPR, (k_omega_rescue_dot<F, L><<<c.gS, dim3(kBlock), 0, st>>>(p->n, (const F *)p->ring, p->slot_stride, S, j, r, part_r, p->om_ticket, p->st, c.orth_tol, om))));
  }
  if (!(part & seq::STEP_TAIL)) return SLQ_OK;
  PROFILED(p, SLQ_K_REORTH_UPD, SLQ_TRY(launch_ring_gen(p, PASS_UPDATEG, r, c.gT, st, j, s.xt_update, false, om.mode == 1 ? om.read + (size_t)j * p->NP : nullptr)));
  PROFILED(p, SLQ_K_FINALIZE,
           hipLaunchKernelGGL(k_fin_beta_gram, dim3((bp + 63) / 64, r + 1), dim3(kFinThreads), 0, st, p->st, p->part, c.blocks(s.blk_beta), j, r, c.residual_tol, om));
  return SLQ_OK;
}

// the same sequence on the generic passes (k_csr_pass<PASS_UPDATEG>; r04): alpha-only pass over the upper triangle, projections from Gram rows
static int launch_gram_csr(const RunFrame &c, const seq::StepShape &s, int j, int part) {
  slq_plan *p = c.p;
  hipStream_t st = c.st;
  const int bp = p->bpad, r = s.r;
  if (part & seq::STEP_FRONT) {
    PROFILED(p, SLQ_K_SPMM, SLQ_TRY(launch_fused_pass<PASS_ALPHA>(c, s, j, 0, c.lds_alpha(s), s.xt_alpha)));
    PROFILED(p, SLQ_K_FINALIZE,
             hipLaunchKernelGGL(k_fin_gram, dim3((bp + 63) / 64, r), dim3(kFinThreads), 0, st, p->st, p->part, c.blocks(s.blk_alpha), j, r, c.orth_tol, c.om_off, (int)(part == seq::STEP_FRONT)));
  }
  if (!(part & seq::STEP_TAIL)) return SLQ_OK;
  PROFILED(p, SLQ_K_REORTH_UPD, DISPATCH(p->dtype, p->LPR, (launch_csr_updateg<F, L>(p, r, s.pipe_on != 0, c.gU, c.lds_fused(s), st, j, s.xt_update))));
  PROFILED(p, SLQ_K_FINALIZE,
           hipLaunchKernelGGL(k_fin_beta_gram, dim3((bp + 63) / 64, r + 1), dim3(kFinThreads), 0, st, p->st, p->part, c.blocks(s.blk_beta), j, r, c.residual_tol, c.om_off));
  return SLQ_OK;
}

// fused passes, r >= 1: alpha comes out of the dots pass (PASS_ADOTS: two gather passes per step instead of three); the
// stored-u sequence is this one with the bits that make the first pass store u and the second read it back
static int launch_merged(const RunFrame &c, const seq::StepShape &s, int j, int part) {
  slq_plan *p = c.p;
  const int bp = p->bpad, r = s.r;
  if (part & seq::STEP_FRONT) {
    PROFILED(p, SLQ_K_REORTH_DOT, SLQ_TRY(launch_fused_pass<PASS_ADOTS>(c, s, j, r, c.lds_fused(s), s.xt_dots)));
    PROFILED(p, SLQ_K_FINALIZE,
             hipLaunchKernelGGL(k_fin_adots, dim3((bp + 63) / 64, r), dim3(kFinThreads), 0, c.st, p->st, p->part, c.blocks(s.blk_dots), j, r, c.orth_tol, (int)(part == seq::STEP_FRONT)));
  }
  if (!(part & seq::STEP_TAIL)) return SLQ_OK;
  PROFILED(p, SLQ_K_REORTH_UPD, SLQ_TRY(launch_fused_pass<PASS_UPDATE>(c, s, j, r, c.lds_fused(s), s.xt_update)));
  return SLQ_OK;
}

// fused passes with the alpha pass on its own (r == 0, or SLQ_MERGED=0): alpha, dots (r > 0), update
static int launch_separate(const RunFrame &c, const seq::StepShape &s, int j, int part) {
  slq_plan *p = c.p;
  const int bp = p->bpad, r = s.r;
  if (part & seq::STEP_FRONT) {
    PROFILED(p, SLQ_K_SPMM, SLQ_TRY(launch_fused_pass<PASS_ALPHA>(c, s, j, 0, c.lds_alpha(s), s.xt_alpha)));
    PROFILED(p, SLQ_K_FINALIZE,
             hipLaunchKernelGGL(k_fin_alpha, c.gF, dim3(kFinThreads), 0, c.st, p->st, p->part, c.blocks(s.blk_alpha), j, s.xt_alpha & 1, (int)(part == seq::STEP_FRONT)));
  }
  if ((part & seq::STEP_FRONT) && r > 0) {
    PROFILED(p, SLQ_K_REORTH_DOT, SLQ_TRY(launch_fused_pass<PASS_DOTS>(c, s, j, r, c.lds_fused(s), s.xt_dots)));
    PROFILED(p, SLQ_K_FINALIZE,
             hipLaunchKernelGGL(k_fin_gamma, dim3((bp + 63) / 64, r), dim3(kFinThreads), 0, c.st, p->st, p->part, c.blocks(s.blk_dots), j, 0, c.orth_tol));
  }
  if (!(part & seq::STEP_TAIL)) return SLQ_OK;
  PROFILED(p, (r == 0 ? SLQ_K_AXPY_NORM : SLQ_K_REORTH_UPD), SLQ_TRY(launch_fused_pass<PASS_UPDATE>(c, s, j, r, c.lds_fused(s), s.xt_update)));
  return SLQ_OK;
}

// the sweeps' first launch: W_n = A W_c - (three-term part) with the alpha partials, by the kernel of the operator's kind.
// cheb: a Chebyshev step - no k_fin_alpha (nothing reads the alpha partials), and the unfused product's epilogue is
// k_cheb_3term, which closes the step's vector work; after the other products the caller runs k_cheb_axpy
static int launch_sweep_product(const RunFrame &c, const seq::StepShape &s, int j, bool cheb = false) {
  slq_plan *p = c.p;
  const slq_operator *op = p->op;
  hipStream_t st = c.st;
  const int bp = p->bpad, S = p->S;
  const int sc_ = j % S, sp_ = (j + S - 1) % S, sn_ = (j + 1) % S;
  const int first = (j == 0);
  int nblk = c.blocks(s.blk_alpha);
  switch (s.product) {
    case seq::PRODUCT_RING:
      // the sweeps' SpMM + three-term step on the ring-fed tiles (k_csr_ring_pass<PASS_SPMM>): same result slot, same alpha partials
      PROFILED(p, SLQ_K_SPMM, {
        if (s.gen) SLQ_TRY(launch_ring_gen(p, PASS_SPMM, 0, c.gT, st, j, 0, false));
        else if (c.nt) DISPATCH(p->dtype, p->LPR, (launch_tile_pass<F, L, PASS_SPMM, 1, 0>(p, c.gT, 0, st, j, 0, false)));
        else DISPATCH(p->dtype, p->LPR, (launch_tile_pass<F, L, PASS_SPMM, 0, 0>(p, c.gT, 0, st, j, 0, false)));
      });
      break;
    case seq::PRODUCT_CSR: {
      const size_t spmm_pad = (size_t)p->sw.spmm_pad;  // dynamic LDS only to cap residency at 2 per CU (panel after panel: 38.8 -> 34.7 ms per 26 launches at orth 30)
#define SPMM_LAUNCH(LP, SP)                                                                          \
  DISPATCH(p->dtype, p->LPR,                                                                         \
           (k_spmm_3term<F, L, LP, SP><<<c.gA, dim3(kBlock), spmm_pad, st>>>(                        \
               p->n, op->csr.rp(), op->csr.ci(), op->csr.vals.as<const F>(), (const F *)slot_ptr(p, sc_),       \
               (const F *)slot_ptr(p, sp_), (F *)slot_ptr(p, sn_), p->st.coefA, p->part, bp, first)))
      PROFILED(p, SLQ_K_SPMM, {
        switch (c.nt ? 11 : 0) {  // tens digit: load policy, units: store policy
          case 1: SPMM_LAUNCH(0, 1); break;
          case 2: SPMM_LAUNCH(0, 2); break;
          case 10: SPMM_LAUNCH(1, 0); break;
          case 11: SPMM_LAUNCH(1, 1); break;
          case 12: SPMM_LAUNCH(1, 2); break;
          default: SPMM_LAUNCH(0, 0); break;
        }
      });
#undef SPMM_LAUNCH
      break;
    }
    case seq::PRODUCT_DENSE:
      PROFILED(p, SLQ_K_SPMM, SLQ_TRY(launch_dense_mfma(p, slot_ptr(p, sc_), slot_ptr(p, sp_), slot_ptr(p, sn_), first, 0, &nblk)));
      break;
    default:
      SLQ_TRY(apply_operator_unfused(p, sc_));
      if (cheb)
        PROFILED(p, SLQ_K_AXPY_NORM,
                 DISPATCH(p->dtype, p->LPR,
                          (k_cheb_3term<F, L><<<c.gS, dim3(kBlock), 0, st>>>(p->n, (const F *)p->T, (const F *)slot_ptr(p, sc_), (const F *)slot_ptr(p, sp_),
                                                                             (F *)slot_ptr(p, sn_), p->st.coefA, p->st.coefB, p->part, bp, first))));
      else
      PROFILED(p, SLQ_K_AXPY_NORM,
               DISPATCH(p->dtype, p->LPR,
                        (k_3term<F, L><<<c.gS, dim3(kBlock), 0, st>>>(p->n, (const F *)p->T, (const F *)slot_ptr(p, sc_), (const F *)slot_ptr(p, sp_),
                                                                      (F *)slot_ptr(p, sn_), p->st.coefA, p->part, bp, first))));
      break;
  }
  if (cheb) return SLQ_OK;
  PROFILED(p, SLQ_K_FINALIZE, hipLaunchKernelGGL(k_fin_alpha, c.gF, dim3(kFinThreads), 0, st, p->st, p->part, nblk, j, 0, 0));
  return SLQ_OK;
}

// store-and-revisit sweeps: the product, then the reorthogonalisation against the r ring columns in the order the shape names
static int launch_sweeps(const RunFrame &c, const seq::StepShape &s, int j) {
  slq_plan *p = c.p;
  hipStream_t st = c.st;
  const int bp = p->bpad, S = p->S, r = s.r;
  SLQ_TRY(launch_sweep_product(c, s, j));
  if (s.seq == seq::SEQ_SWEEPS_PLAIN) {
    PROFILED(p, SLQ_K_AXPY_NORM,
             DISPATCH(p->dtype, p->LPR,
                      (k_axpy_norm<F, L, 0><<<c.gS, dim3(kBlock), 0, st>>>(p->n, (F *)slot_ptr(p, (j + 1) % S), (const F *)slot_ptr(p, j % S), p->st.coefB, p->part, bp))));
  } else if (s.seq == seq::SEQ_SWEEPS_MGS) {
    for (int i = 0; i < r; ++i) {
      PROFILED(p, SLQ_K_REORTH_DOT,
               DISPATCH(p->dtype, p->LPR,
                        (k_reorth_dot<F, L><<<c.gS, dim3(kBlock), 0, st>>>(p->n, (F *)p->ring, p->slot_stride, S, j, i, 1, (int)(i == 0), p->st.coefB, p->part, bp))));
      PROFILED(p, SLQ_K_FINALIZE,
               hipLaunchKernelGGL(k_fin_gamma, dim3((bp + 63) / 64, 1), dim3(kFinThreads), 0, st, p->st, p->part, p->nblkS, j, i, c.orth_tol));
      SLQ_TRY(launch_reorth_update_range(p, j, i, i + 1));
    }
  } else {
    for (int i0 = 0; i0 < r; i0 += kReorthChunk) {  // reorth columns per dots launch
      const int rc = std::min(kReorthChunk, r - i0);
      PROFILED(p, SLQ_K_REORTH_DOT, DISPATCH(p->dtype, p->LPR, (launch_reorth_dot<F, L>(p, c.gS, st, j, i0, rc))));
      PROFILED(p, SLQ_K_FINALIZE,
               hipLaunchKernelGGL(k_fin_gamma, dim3((bp + 63) / 64, rc), dim3(kFinThreads), 0, st, p->st, p->part, p->nblkS, j, i0, c.orth_tol));
    }
    SLQ_TRY(launch_reorth_update(p, j, r, 0, p->sw.defer_axpy));
  }
  return SLQ_OK;
}

// enqueue the launch sequence of steps [j0, j1) on the context stream (also run under stream capture). Between steps the whole
// state of a run lives on the device; the host carries p->prev_xt, read here at j0 and left as step j1 - 1 sets it.
// What a step launches is step_shape's answer (slq_sequence.hpp); the functions above launch it and decide nothing.
static RunFrame run_frame(slq_plan *p, double rtol) {
  const int bp = p->bpad;
  RunFrame c;
  c.p = p, c.st = p->ctx->stream, c.nt = p->sw.nt != 0;
  c.eps = p->dtype == SLQ_F64 ? std::numeric_limits<double>::epsilon() : (double)std::numeric_limits<float>::epsilon();
  c.residual_tol = std::sqrt((double)p->n) * rtol;   // lanczos.h:110
  c.orth_tol = 2.0 * c.eps * std::sqrt((double)p->n);  // lanczos.h:53
  c.gA = dim3(p->nblkA, p->NP), c.gS = dim3(p->nblkS, p->NP), c.gU = dim3(p->nblkU, p->NP), c.gF = dim3((bp + 63) / 64);
  c.gAf = dim3(p->nblkF, p->NP), c.gT = dim3(p->nblkT, p->NP);
  c.lds0 = sizeof(double) * kWaves * 64 * (p->dtype == SLQ_F64 ? 2 : 4);
  memset(&c.om_off, 0, sizeof(c.om_off));
  return c;
}

// one step, or one part of it (seq::StepPart; the sweeps are never split: no plan with a lazy tail closes on them)
static int launch_step(const RunFrame &c, const seq::StepShape &s, int j, int part) {
  slq_plan *p = c.p;
  switch (s.seq) {
    case seq::SEQ_GRAM_RING: return launch_gram_ring(c, s, j, part);  // (k_fin_beta_gram closes the step)
    case seq::SEQ_GRAM_CSR: return launch_gram_csr(c, s, j, part);
    case seq::SEQ_MERGED:
    case seq::SEQ_STORED_U: SLQ_TRY(launch_merged(c, s, j, part)); break;
    case seq::SEQ_SEPARATE: SLQ_TRY(launch_separate(c, s, j, part)); break;
    default:
      if (part != seq::STEP_WHOLE) return fail(SLQ_EINVAL, "internal: a step of the store-and-revisit sweeps has no closing tail");
      SLQ_TRY(launch_sweeps(c, s, j));
      break;
  }
  if (part & seq::STEP_TAIL)
    PROFILED(p, SLQ_K_FINALIZE,
             hipLaunchKernelGGL(k_fin_beta, c.gF, dim3(kFinThreads), 0, c.st, p->st, p->part, c.blocks(s.blk_beta), j, c.residual_tol, s.prev_xt ? 1 : 0));
  return SLQ_OK;
}

// the plan leaves the closing tail of a run that reaches deg to the first entry that asks for it
static bool plan_lazy_tail(const slq_plan *p) { return !p->cheb && seq::has_lazy_tail(sequence_facts(p), p->sw.last_store != 2, !p->facts.affine); }

// lazy_tail: a run that reaches deg launches the front of step deg - 1 only (run_range marks the tail pending)
static int enqueue_run(slq_plan *p, double rtol, int j0, int j1, bool lazy_tail = false) {
  hipStream_t st = p->ctx->stream;
  const int bp = p->bpad, deg = p->deg;
  const RunFrame c = run_frame(p, rtol);
  if (j0 == 0) {
    // alpha and nu[1..] start from zero (the reference's fresh np.zeros buffers, lanczos.py:101-102)
    HIP_TRY(hipMemsetAsync(p->st.alpha, 0, (size_t)(deg + 1) * bp * 8, st));
    HIP_TRY(hipMemsetAsync(p->st.nu + bp, 0, (size_t)deg * bp * 8, st));
    HIP_TRY(hipMemsetAsync(p->st.gram, 0, (size_t)2 * (kFusedMaxR + 1) * bp * 8, st));  // (the Gram rows of a previous run are never read - index guards - but need not be trusted to be)
    if (p->omega_on) {  // the edge recurrence starts with the run (its counters are the caller's to reset: slq_plan_window_columns)
      HIP_TRY(hipMemsetAsync(p->om_buf, 0, (size_t)4 * bp * 8, st));
      HIP_TRY(hipMemsetAsync(p->om_flags, 0, (size_t)2 * (deg + 1) * p->NP * sizeof(int), st));
    }
  }
  if (j0 == 0 && p->om_census) HIP_TRY(hipMemsetAsync(p->om_census, 0, (size_t)(deg + 1) * (kFusedMaxR + 1) * p->NP * sizeof(int), st));
  const seq::SequenceFacts facts = sequence_facts(p);
  bool prev_xt = j0 > 0 && p->prev_xt;  // the previous step's update pass produced the cross term W_{j}.W_{j-1}
  for (int j = j0; j < j1; ++j) {
    const seq::StepShape s = seq::step_shape(facts, j, prev_xt);
    prev_xt = s.prev_xt != 0;
    SLQ_TRY(launch_step(c, s, j, (lazy_tail && j == deg - 1) ? seq::STEP_FRONT : seq::STEP_WHOLE));
  }
  p->prev_xt = prev_xt;
  HIP_TRY(hipGetLastError());
  if (p->launch_error) {
    p->launch_error = false;
    return fail(SLQ_EINVAL, "internal: a pass of the launch sequence had no kernel for this plan's tiles");
  }
  return SLQ_OK;
}

// ---- Chebyshev moments (kernels in slq_cheb.hpp) ------------------------------------------------------
extern "C" int slq_plan_create_chebyshev(slq_context *ctx, slq_operator *op, int nprobes, int nsteps, slq_plan **out) {
  return plan_create_mode(ctx, op, nprobes, nsteps, 0, PlanKind::Chebyshev, out);
}

extern "C" int slq_debug_cheb_step_shape(const int *facts, int nfacts, int j, int *out, int nout) {
  if (!facts || !out || nfacts != seq::kNumFacts || nout != seq::kNumChebShape) return fail(SLQ_EINVAL, "slq_debug_cheb_step_shape: %d facts in, %d values out", seq::kNumFacts, seq::kNumChebShape);
  seq::cheb_shape_to_array(seq::cheb_step_shape(seq::facts_from_array(facts), j), out);
  return SLQ_OK;
}

extern "C" int slq_debug_cheb_action_schedule(int nsteps, int *t0, int *nc, int cap, int *npieces, int *ring_slots_out, int *acc_cols) {
  if (nsteps < 1 || nsteps > kMaxChebSteps || cap < 0 || !npieces)
    return fail(SLQ_EINVAL, "slq_debug_cheb_action_schedule: nsteps = %d must lie in [1, %d], cap >= 0, npieces not NULL", nsteps, kMaxChebSteps);
  *npieces = seq::cheb_action_schedule(nsteps, kChebAccCols, t0, nc, nullptr, cap);
  if (ring_slots_out) *ring_slots_out = seq::cheb_action_ring_slots(nsteps, kChebAccCols);
  if (acc_cols) *acc_cols = kChebAccCols;
  return SLQ_OK;
}

// One accumulation launch of an action: columns t0 .. t0 + nc - 1 of the ring into the output panel, the coefficients in
// cheb_coef (device), the live-column mask from their host copy.
static int launch_cheb_accumulate(slq_plan *p, int t0, int nc, const double *coef_h) {
  hipStream_t st = p->ctx->stream;
  const dim3 gS(p->nblkS, p->NP);
  unsigned live = 0;
  for (int i = 0; i < nc; ++i)
    if (!p->acc_skip || coef_h[t0 + i] != 0.0) live |= 1u << i;
  p->cheb_cols_read += (uint64_t)__builtin_popcount(live);
  p->cheb_cols_offered += (uint64_t)nc;
  PROFILED(p, SLQ_K_COMBINE,
           DISPATCH(p->dtype, p->LPR,
                    (k_cheb_accumulate<F, L><<<gS, dim3(kBlock), 0, st>>>(p->n, (const F *)p->ring, p->slot_stride, p->S, t0, nc, live,
                                                                        (const double *)p->cheb_coef, (F *)slot_ptr(p, p->y_slot), t0 == 0 ? 1 : 0))));
  return SLQ_OK;
}

// Step j is the update pass cheb_step_shape names (or the product kernel and k_cheb_axpy where the plan takes sweeps) and one
// k_fin_cheb: a strict subset of the orth-0 Lanczos step's launches. Enqueued directly on the context stream.
// action_coef: null, or the host copy of the nsteps + 1 coefficients of an action (already in cheb_coef): the accumulation
// launches of seq::cheb_action_piece_after go between the steps.
static int cheb_run(slq_plan *p, const char *who, double center, double halfwidth, double outside_tol, const double *action_coef) {
  if (!p->probes_ready) return fail(SLQ_EINVAL, "%s: set or generate probes first", who);
  SLQ_TRY(precond_check_fresh(p->op, who));
  if (!std::isfinite(center) || !std::isfinite(halfwidth) || !(halfwidth > 0.0))
    return fail(SLQ_EINVAL, "%s: center = %g, halfwidth = %g (finite, halfwidth > 0)", who, center, halfwidth);
  HIP_TRY(hipSetDevice(p->ctx->device));
  hipStream_t st = p->ctx->stream;
  const int bp = p->bpad, S = p->S;
  const RunFrame c = run_frame(p, 0.0);
  const double tol = outside_tol > 0.0 ? outside_tol : kChebOutsideTol;
  const double inv_h = 1.0 / halfwidth, c_over_h = center / halfwidth;
  const int sphere = p->pdf_sphere ? 1 : 0;
  const seq::SequenceFacts facts = sequence_facts(p);
  // mu_0: the probes' norm sweep once more (one read of the panel per run), reduced with the error terms carried (k_fin_cheb)
  PROFILED(p, SLQ_K_AXPY_NORM,
           DISPATCH(p->dtype, p->LPR,
                    (k_axpy_norm<F, L, 1><<<c.gS, dim3(kBlock), 0, st>>>(p->n, (F *)slot_ptr(p, 0), (const F *)nullptr, (const double *)nullptr, p->part, bp))));
  PROFILED(p, SLQ_K_FINALIZE,
           hipLaunchKernelGGL(k_fin_cheb, c.gF, dim3(kFinThreads), 0, st, p->st, p->part, p->nblkS, -1, p->cheb_mu, p->cheb_out, inv_h, c_over_h, tol, sphere));
  int c0 = 0;  // the oldest unconsumed column of an action
  for (int j = 0; j < p->deg; ++j) {
    const seq::ChebStepShape s = seq::cheb_step_shape(facts, j);
    seq::StepShape l;  // (what the launchers of the Lanczos step read of a shape)
    l.tiled = s.tiled, l.gen = s.gen, l.pipe_on = s.pipe_on, l.product = s.product, l.blk_alpha = s.blk_product;
    int nblk = c.blocks(s.blk);
    if (!s.sweeps) {
      PROFILED(p, SLQ_K_AXPY_NORM, SLQ_TRY(launch_fused_pass<PASS_UPDATE>(c, l, j, 0, c.lds_fused(l), s.xt_update)));
    } else {
      SLQ_TRY(launch_sweep_product(c, l, j, true));
      if (s.product != seq::PRODUCT_UNFUSED)
        PROFILED(p, SLQ_K_AXPY_NORM,
                 DISPATCH(p->dtype, p->LPR,
                          (k_cheb_axpy<F, L><<<c.gS, dim3(kBlock), 0, st>>>(p->n, (F *)slot_ptr(p, (j + 1) % S), (const F *)slot_ptr(p, j % S), p->st.coefB, p->part, bp))));
      nblk = p->nblkS;
    }
    PROFILED(p, SLQ_K_FINALIZE,
             hipLaunchKernelGGL(k_fin_cheb, c.gF, dim3(kFinThreads), 0, st, p->st, p->part, nblk, j, p->cheb_mu, p->cheb_out, inv_h, c_over_h, tol, sphere));
    if (action_coef) {
      const int m = seq::cheb_action_piece_after(p->deg, p->acc_cols, j, c0);
      if (m) SLQ_TRY(launch_cheb_accumulate(p, c0, m, action_coef));
      c0 += m;
    }
  }
  HIP_TRY(hipGetLastError());
  p->probes_ready = false;
  p->cheb_ran = true;
  p->cheb_c = center, p->cheb_h = halfwidth;
  if (p->launch_error) {
    p->launch_error = false;
    p->cheb_ran = false;
    return fail(SLQ_EINVAL, "internal: a pass of the launch sequence had no kernel for this plan's tiles");
  }
  return SLQ_OK;
}

extern "C" int slq_plan_run_chebyshev(slq_plan *p, double center, double halfwidth, double outside_tol) {
  if (!p) return fail(SLQ_EINVAL, "plan is NULL");
  SLQ_TRY(need_chebyshev(p, "slq_plan_run_chebyshev"));
  return cheb_run(p, "slq_plan_run_chebyshev", center, halfwidth, outside_tol, nullptr);
}

// the outside flags and the ring bail-out word of the last Chebyshev run (synchronises); *raised = probes whose flag is up
static int cheb_flags(slq_plan *p, std::vector<int> &flags, int *raised) {
  hipStream_t st = p->ctx->stream;
  flags.assign((size_t)p->nprobes, 0);
  int ring_bad = 0;
  HIP_TRY(hipMemcpyAsync(flags.data(), p->cheb_out, (size_t)p->nprobes * sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&ring_bad, p->ring_fail_d, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  SLQ_TRY(ring_flag_status(ring_bad));
  *raised = 0;
  for (int f : flags) *raised += f != 0;
  return SLQ_OK;
}
static int cheb_outside_error(const slq_plan *p, const char *who, int raised) {
  return fail(SLQ_EINVAL, "%s: %d of %d probes saw a moment above mu_0: the spectrum is not inside the bounds [%.17g, %.17g] of the run", who, raised,
              p->nprobes, p->cheb_c - p->cheb_h, p->cheb_c + p->cheb_h);
}

// ---- the Chebyshev action Y = sum_k c_k T_k(A~) X ---------------------------------------------------
extern "C" int slq_plan_create_chebyshev_action(slq_context *ctx, slq_operator *op, int nprobes, int nsteps, slq_plan **out) {
  return plan_create_mode(ctx, op, nprobes, nsteps, 0, PlanKind::ChebyshevAction, out);
}

// the run with its accumulation launches; on SLQ_OK the output panel y_slot holds the action and no `outside` flag is up
static int cheb_action_device(slq_plan *p, const char *who, double center, double halfwidth, double outside_tol, int ncoef, const double *coef) {
  SLQ_TRY(need_chebyshev(p, who));
  if (!p->cheb_action) return fail(SLQ_EINVAL, "%s: not an action plan (slq_plan_create_chebyshev_action)", who);
  if (!p->probes_ready) return fail(SLQ_EINVAL, "%s: set or generate probes first", who);
  if (ncoef != p->deg + 1) return fail(SLQ_EINVAL, "%s: ncoef = %d, a plan of %d steps takes %d coefficients", who, ncoef, p->deg, p->deg + 1);
  if (!coef) return fail(SLQ_EINVAL, "%s: coef is NULL", who);
  for (int k = 0; k < ncoef; ++k)
    if (!std::isfinite(coef[k])) return fail(SLQ_EINVAL, "%s: coefficient %d is not finite", who, k);
  // sphere probes drawn on the device are sqrt(n) g / ||g|| while the panel holds g (k_fin_init): the moments carry the ratio,
  // the vectors of the ring do not
  if (p->pdf_sphere)
    return fail(SLQ_EINVAL, "%s: the probes are sphere probes drawn on the device, whose panel holds the normal draw g, not the probe: set them with slq_plan_set_probes", who);
  HIP_TRY(hipSetDevice(p->ctx->device));
  HIP_TRY(hipMemcpyAsync(p->cheb_coef, coef, (size_t)ncoef * 8, hipMemcpyHostToDevice, p->ctx->stream));
  SLQ_TRY(cheb_run(p, who, center, halfwidth, outside_tol, coef));
  std::vector<int> flags;
  int raised = 0;
  SLQ_TRY(cheb_flags(p, flags, &raised));  // (synchronises)
  if (raised) return cheb_outside_error(p, who, raised);
  return SLQ_OK;
}

extern "C" int slq_plan_chebyshev_action(slq_plan *p, double center, double halfwidth, double outside_tol, int ncoef, const double *coef, void *Y,
                                         int64_t ldy) {
  if (!p || !Y) return fail(SLQ_EINVAL, "plan/Y is NULL");
  if (ldy < p->n) return fail(SLQ_EINVAL, "slq_plan_chebyshev_action: ldy < n");
  SLQ_TRY(cheb_action_device(p, "slq_plan_chebyshev_action", center, halfwidth, outside_tol, ncoef, coef));
  return panel_to_host(p, p->y_slot, 0, p->nprobes, Y, ldy, nullptr);
}

extern "C" int slq_plan_get_moments(slq_plan *p, double *mu, int *outside) {
  if (!p) return fail(SLQ_EINVAL, "plan is NULL");
  SLQ_TRY(need_chebyshev(p, "slq_plan_get_moments"));
  if (!p->cheb_ran) return fail(SLQ_EINVAL, "slq_plan_get_moments: no completed run");
  HIP_TRY(hipSetDevice(p->ctx->device));
  hipStream_t st = p->ctx->stream;
  const int bp = p->bpad, P = p->nprobes;
  const size_t K = (size_t)2 * p->deg + 1;
  std::vector<double> h;
  if (mu) {
    h.resize(K * bp);
    HIP_TRY(hipMemcpyAsync(h.data(), p->cheb_mu, h.size() * 8, hipMemcpyDeviceToHost, st));
  }
  std::vector<int> flags;
  int raised = 0;
  SLQ_TRY(cheb_flags(p, flags, &raised));
  if (mu)
    for (int i = 0; i < P; ++i)
      for (size_t k = 0; k < K; ++k) mu[(size_t)i * K + k] = h[k * bp + i];
  if (outside) memcpy(outside, flags.data(), (size_t)P * sizeof(int));
  return SLQ_OK;
}

extern "C" int slq_plan_moment_sum(slq_plan *p, int ncoef, const double *coef, double *quad, double *stage) {
  if (!p || !coef) return fail(SLQ_EINVAL, "plan/coef is NULL");
  SLQ_TRY(need_chebyshev(p, "slq_plan_moment_sum"));
  if (!p->cheb_ran) return fail(SLQ_EINVAL, "slq_plan_moment_sum: no completed run");
  const int K = 2 * p->deg + 1, P = p->nprobes;
  if (ncoef < 1 || ncoef > K) return fail(SLQ_EINVAL, "slq_plan_moment_sum: ncoef = %d must lie in [1, %d] (2 nsteps + 1 moments)", ncoef, K);
  HIP_TRY(hipSetDevice(p->ctx->device));
  hipStream_t st = p->ctx->stream;
  std::vector<int> flags;
  int raised = 0;
  SLQ_TRY(cheb_flags(p, flags, &raised));
  if (raised) return cheb_outside_error(p, "slq_plan_moment_sum", raised);
  double *stage_d = p->cheb_coef + K;
  HIP_TRY(hipMemcpyAsync(p->cheb_coef, coef, (size_t)ncoef * 8, hipMemcpyHostToDevice, st));
  PROFILED(p, SLQ_K_QUADRATURE,
           hipLaunchKernelGGL(k_moment_sum, dim3((P + 63) / 64), dim3(64), 0, st, P, p->bpad, ncoef, (const double *)p->cheb_coef, (const double *)p->cheb_mu, p->quad_d));
  if (stage)
    hipLaunchKernelGGL(k_stage_reduce, dim3(1), dim3(kStageThreads), 0, st, P, (const double *)p->quad_d, (const double *)nullptr, stage_d);
  HIP_TRY(hipGetLastError());
  if (quad) HIP_TRY(hipMemcpyAsync(quad, p->quad_d, (size_t)P * 8, hipMemcpyDeviceToHost, st));
  if (stage) HIP_TRY(hipMemcpyAsync(stage, stage_d, 4 * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return SLQ_OK;
}

static int run_range(slq_plan *p, double rtol, int j0, int j1);

extern "C" int slq_plan_run(slq_plan *p, double rtol) {
  if (!p) return fail(SLQ_EINVAL, "plan is NULL");
  SLQ_TRY(need_lanczos(p, "slq_plan_run"));
  if (!p->probes_ready) return fail(SLQ_EINVAL, "slq_plan_run: set or generate probes first");
  return run_range(p, rtol, 0, p->deg);
}

extern "C" int slq_plan_run_steps(slq_plan *p, double rtol, int upto) {
  if (!p) return fail(SLQ_EINVAL, "plan is NULL");
  SLQ_TRY(need_lanczos(p, "slq_plan_run_steps"));
  if (p->nstale > 0) return fail(SLQ_EINVAL, "slq_plan_run_steps: a plan with stale ring columns is not resumable");
  if (p->basis_mode == 2) return fail(SLQ_EINVAL, "slq_plan_run_steps: a recompute plan runs in one piece (a staged two-pass run is not supported)");
  const bool fresh = p->probes_ready;  // (probes set or generated and not yet consumed: cur == 0)
  if (!fresh && !(p->ran && p->cur > 0)) return fail(SLQ_EINVAL, "slq_plan_run_steps: set or generate probes first");
  const int cur = fresh ? 0 : p->cur;
  if (upto <= cur || upto > p->deg) return fail(SLQ_EINVAL, "slq_plan_run_steps: upto = %d must lie in (%d, %d] (steps done, the plan's deg)", upto, cur, p->deg);
  if (!fresh && rtol != p->run_rtol) return fail(SLQ_EINVAL, "slq_plan_run_steps: rtol = %g differs from the %g this run began with", rtol, p->run_rtol);
  return run_range(p, rtol, cur, upto);
}

extern "C" int slq_plan_steps_done(const slq_plan *p, int *cur) {
  if (!p || !cur) return fail(SLQ_EINVAL, "plan/cur is NULL");
  *cur = p->probes_ready ? 0 : (p->ran ? p->cur : 0);
  return SLQ_OK;
}

constexpr size_t kGraphCacheMax = 16;
// What can change under a live plan and changes the launch sequence: the number of stale ring columns, and whether the plan's kernel
// operator has a diagonal scale - k_kernel_panel_scaled is another kernel than k_kernel_panel, so a graph captured in one state must not
// be replayed in the other. New VALUES of the scale need no new graph: the kernel reads them from a fixed address.
static unsigned graph_variant(const slq_plan *p) {
  return (unsigned)p->nstale | (p->op->kind == OP_KERNEL && p->op->k_scaled ? 0x80000000u : 0u);
}

static int run_range(slq_plan *p, double rtol, int j0, int j1) {
  SLQ_TRY(precond_check_fresh(p->op, "slq_plan_run"));
  HIP_TRY(hipSetDevice(p->ctx->device));
  hipStream_t st = p->ctx->stream;
  // The launch sequence of a run (7 launches per Lanczos step, ~210 for k = 30) depends only on
  // the plan, so it is captured into a hipGraph once and replayed: launch-bound for small n,
  // a few per cent for n = 1e6. Not used while per-kernel events are recorded, nor for host-callback
  // operators (they synchronise with the host every step).
  const bool graph_ok = p->sw.graph && !p->prof && p->op->kind != OP_CALLBACK && p->op->kind != OP_DEVICE_CALLBACK;
  // the stage that reaches deg leaves its closing tail out, of the captured graph too (the key does not change: whether a plan has
  // a lazy tail follows from the plan's switches and from nstale, which is the key's variant); a flush launches it directly
  // (a run from step 0 needs new probes, and init_from_probes has dropped what the run before left pending)
  const bool lazy_tail = j1 == p->deg && plan_lazy_tail(p);
  if (!graph_ok) {
    SLQ_TRY(enqueue_run(p, rtol, j0, j1, lazy_tail));
  } else {
    const unsigned variant = graph_variant(p);
    size_t gi = 0;
    for (; gi < p->graphs.size(); ++gi) {
      const auto &g = p->graphs[gi];
      if (g.j0 == j0 && g.j1 == j1 && g.rtol == rtol && g.variant == variant) break;
    }
    if (gi == p->graphs.size()) {
      // a graph of the same steps for another rtol or variant is replaced (as the one-shot graph always was); a full cache
      // gives up its oldest entry
      for (size_t k = 0; k < p->graphs.size();) {
        if (p->graphs[k].j0 == j0 && p->graphs[k].j1 == j1) {
          HIP_TRY(hipGraphExecDestroy(p->graphs[k].exec));
          p->graphs.erase(p->graphs.begin() + k);
        } else {
          ++k;
        }
      }
      if (p->graphs.size() >= kGraphCacheMax) {
        HIP_TRY(hipGraphExecDestroy(p->graphs.front().exec));
        p->graphs.erase(p->graphs.begin());
      }
      hipGraph_t graph = nullptr;
      const bool xt_in = p->prev_xt;
      HIP_TRY(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
      const int rc = enqueue_run(p, rtol, j0, j1, lazy_tail);
      hipError_t ce = hipStreamEndCapture(st, &graph);
      if (rc != SLQ_OK) {
        if (graph) hipGraphDestroy(graph);
        p->prev_xt = xt_in;
        return rc;
      }
      if (ce != hipSuccess) return fail(SLQ_EHIP, "hipStreamEndCapture: %s", hipGetErrorString(ce));
      hipGraphExec_t exec = nullptr;
      ce = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
      hipGraphDestroy(graph);
      if (ce != hipSuccess) {
        p->prev_xt = xt_in;
        return fail(SLQ_EHIP, "hipGraphInstantiate: %s", hipGetErrorString(ce));
      }
      p->graphs.push_back({j0, j1, rtol, variant, exec, p->prev_xt});
      gi = p->graphs.size() - 1;
    }
    HIP_TRY(hipGraphLaunch(p->graphs[gi].exec, st));
    p->prev_xt = p->graphs[gi].xt_out;
  }
  p->probes_ready = false;
  p->ran = true;
  p->cur = j1;
  p->run_rtol = rtol;
  p->rule_src = 0;
  if (lazy_tail) {
    p->closing.pending = true;
    p->closing.j = p->deg - 1;
    p->closing.rtol = rtol;
    p->closing.shape = seq::step_shape(sequence_facts(p), p->deg - 1, false);  // (prev_xt enters the alpha pass's word only: the front's)
  }
  return SLQ_OK;
}

// The closing tail of the last run, launched now: on the plan's stream, the launches the run would have made behind the front of
// step deg - 1 (same kernels, same arguments, PROFILED like them), directly - a graph of two launches saves nothing. Called by
// every entry that reads what they write: nu[deg], steps and active of the stop rule at deg, the Gram row and sc / cp behind
// it, the edge recurrence's counters of that step.
static int flush_closing_tail(slq_plan *p) {
  if (!p->closing.pending) return SLQ_OK;
  HIP_TRY(hipSetDevice(p->ctx->device));
  const RunFrame c = run_frame(p, p->closing.rtol);
  const int rc = launch_step(c, p->closing.shape, p->closing.j, seq::STEP_TAIL);
  if (rc != SLQ_OK) return rc;
  HIP_TRY(hipGetLastError());
  if (p->launch_error) {
    p->launch_error = false;
    return fail(SLQ_EINVAL, "internal: a pass of the launch sequence had no kernel for this plan's tiles");
  }
  p->closing.pending = false;
  return SLQ_OK;
}

extern "C" int slq_plan_closing_state(slq_plan *p, int *lazy, int *pending) {
  if (!p) return fail(SLQ_EINVAL, "plan is NULL");
  if (lazy) *lazy = plan_lazy_tail(p) ? 1 : 0;
  if (pending) *pending = p->closing.pending ? 1 : 0;
  return SLQ_OK;
}

// has_lazy_tail() of slq_sequence.hpp on facts given as slq_debug_step_shape takes them: no HIP call
extern "C" int slq_debug_lazy_tail(const int *facts, int nfacts, int lazy_close, int values_fixed, int *out) {
  if (!facts || !out || nfacts != seq::kNumFacts) return fail(SLQ_EINVAL, "slq_debug_lazy_tail: %d facts in, one value out", seq::kNumFacts);
  *out = seq::has_lazy_tail(seq::facts_from_array(facts), lazy_close, values_fixed) ? 1 : 0;
  return SLQ_OK;
}

// the entries that mean "the finished run": not while a staged run stands between two stages
static int need_finished_run(const slq_plan *p, const char *who) {
  if (!p->ran) return fail(SLQ_EINVAL, "%s: no completed run", who);
  if (p->cur < p->deg)
    return fail(SLQ_EINVAL, "%s: the run stands at step %d of %d (slq_plan_run_steps); use slq_plan_quadrature_at for a prefix, or run to deg", who, p->cur, p->deg);
  return SLQ_OK;
}

extern "C" int slq_plan_get_tridiag(slq_plan *p, void *alpha, void *beta, int32_t *steps) {
  if (!p) return fail(SLQ_EINVAL, "plan is NULL");
  SLQ_TRY(need_lanczos(p, "slq_plan_get_tridiag"));
  if (!p->ran) return fail(SLQ_EINVAL, "slq_plan_get_tridiag: no completed run");
  HIP_TRY(hipSetDevice(p->ctx->device));
  SLQ_TRY(flush_closing_tail(p));  // (beta_deg, steps)
  hipStream_t st = p->ctx->stream;
  const int bp = p->bpad, deg = p->deg, P = p->nprobes;
  std::vector<double> ha((size_t)(deg + 1) * bp), hn((size_t)(deg + 1) * bp);
  std::vector<int> hs(bp);
  HIP_TRY(hipMemcpyAsync(ha.data(), p->st.alpha, ha.size() * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(hn.data(), p->st.nu, hn.size() * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(hs.data(), p->st.steps, (size_t)bp * 4, hipMemcpyDeviceToHost, st));
  int ring_bad = 0;
  HIP_TRY(hipMemcpyAsync(&ring_bad, p->ring_fail_d, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  SLQ_TRY(ring_flag_status(ring_bad));
  for (int i = 0; i < P; ++i) {
    for (int t = 0; t <= deg; ++t) {
      const double a = ha[(size_t)t * bp + i];
      const double b = (t == 0) ? 0.0 : hn[(size_t)t * bp + i];  // beta[0] = 0 (lanczos.h:121)
      if (p->dtype == SLQ_F64) {
        if (alpha) ((double *)alpha)[(size_t)i * (deg + 1) + t] = a;
        if (beta) ((double *)beta)[(size_t)i * (deg + 1) + t] = b;
      } else {
        if (alpha) ((float *)alpha)[(size_t)i * (deg + 1) + t] = (float)a;
        if (beta) ((float *)beta)[(size_t)i * (deg + 1) + t] = (float)b;
      }
    }
    if (steps) steps[i] = hs[i];
  }
  return SLQ_OK;
}

extern "C" int slq_plan_quadrature(slq_plan *p, int fun_id, const double *fun_params, double *quad,
                                   double *nodes, double *weights) {
  if (!p) return fail(SLQ_EINVAL, "plan is NULL");
  SLQ_TRY(need_lanczos(p, "slq_plan_quadrature"));
  SLQ_TRY(need_finished_run(p, "slq_plan_quadrature"));
  if (fun_id < SLQ_FUN_NONE || fun_id > SLQ_FUN_SOFTSIGN) return fail(SLQ_EINVAL, "Unknown function id %d.", fun_id);
  HIP_TRY(hipSetDevice(p->ctx->device));
  hipStream_t st = p->ctx->stream;
  const int deg = p->deg, P = p->nprobes;
  const double p0 = fun_params ? fun_params[0] : 0.0, p1 = fun_params ? fun_params[1] : 0.0;
  if (p->rule_src == 2) {
    // slq_density_update already ran the QL of this run: only the reduction over the stored rule
    hipLaunchKernelGGL(k_rule_reduce, dim3((P + 63) / 64), dim3(64), 0, st, P, deg, p->nodes_d, p->weights_d, p->st.vnorm2, fun_id, p0,
                       p1, p->quad_d);
  } else {
    const QuadShape q = quadrature_shape(deg, P);
    if (q.lds > 48 * 1024)
      HIP_TRY(hipFuncSetAttribute((const void *)k_quadrature, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIP_TRY(hipMemsetAsync(p->fail_d, 0, sizeof(int), st));
    // (the rule always lands in nodes_d / weights_d: a density update of the same run then needs no QL of its own)
    PROFILED(p, SLQ_K_QUADRATURE,
             hipLaunchKernelGGL(k_quadrature, dim3(q.grid), dim3(64), q.lds, st, p->st, q.lanes, fun_id, p0, p1,
                                p->quad_d, p->nodes_d, p->weights_d, p->fail_d));
  }
  HIP_TRY(hipGetLastError());
  int bad3[3] = {0, 0, 0};  // fail_d[0..2]: the QL of this call, the ring bail-out word, the QL of a density update
  HIP_TRY(hipMemcpyAsync(bad3, p->fail_d, 3 * sizeof(int), hipMemcpyDeviceToHost, st));
  if (quad) HIP_TRY(hipMemcpyAsync(quad, p->quad_d, (size_t)P * 8, hipMemcpyDeviceToHost, st));
  if (nodes) HIP_TRY(hipMemcpyAsync(nodes, p->nodes_d, (size_t)P * deg * 8, hipMemcpyDeviceToHost, st));
  if (weights) HIP_TRY(hipMemcpyAsync(weights, p->weights_d, (size_t)P * deg * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const int bad = p->rule_src == 2 ? bad3[2] : bad3[0];
  if (p->rule_src != 2) {
    p->rule_src = 1;
    p->rule_fail_h = bad ? 1 : 0;
  }
  SLQ_TRY(ring_flag_status(bad3[1]));
  if (bad) return fail(SLQ_ENOTCONV, "tridiagonal QL did not converge for at least one probe");
  return SLQ_OK;
}

// Quadrature of the first m steps of the run as it stands (m <= steps done): rule 0 the m-point Gauss rule - what a run
// of degree m returns -, rule 1 the (m + 1)-point Gauss-Radau rule with a node at `endpoint` (slq_radau.hpp). The rule goes
// to buffers of its own: the finished run's rule (nodes_d / weights_d, shared with slq_density_update) is not touched.
extern "C" int slq_plan_quadrature_at(slq_plan *p, int m, int rule, double endpoint, int fun_id, const double *fun_params,
                                      double *quad, double *nodes, double *weights, double *stage) {
  if (!p) return fail(SLQ_EINVAL, "plan is NULL");
  SLQ_TRY(need_lanczos(p, "slq_plan_quadrature_at"));
  if (!p->ran || p->cur < 1) return fail(SLQ_EINVAL, "slq_plan_quadrature_at: no steps done");
  if (m < 1 || m > p->cur) return fail(SLQ_EINVAL, "slq_plan_quadrature_at: m = %d must lie in [1, %d] (steps done)", m, p->cur);
  if (rule != 0 && rule != 1) return fail(SLQ_EINVAL, "slq_plan_quadrature_at: rule %d (0 Gauss, 1 Gauss-Radau)", rule);
  if (rule == 1 && !std::isfinite(endpoint)) return fail(SLQ_EINVAL, "slq_plan_quadrature_at: the Gauss-Radau rule needs a finite endpoint");
  if (fun_id < SLQ_FUN_NONE || fun_id > SLQ_FUN_SOFTSIGN) return fail(SLQ_EINVAL, "Unknown function id %d.", fun_id);
  HIP_TRY(hipSetDevice(p->ctx->device));
  hipStream_t st = p->ctx->stream;
  const int deg = p->deg, P = p->nprobes, kout = m + rule;
  const size_t rule_sz = (size_t)P * (deg + 1);
  if (!p->at_d) {
    hipError_t e = hipMalloc((void **)&p->at_d, (2 * (size_t)P + 4 + 2 * rule_sz) * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&p->at_flags, 2 * sizeof(int));
    if (e != hipSuccess) {
      if (p->at_d) hipFree(p->at_d);
      p->at_d = nullptr;
      return fail(SLQ_ENOMEM, "slq_plan_quadrature_at: scratch: %s", hipGetErrorString(e));
    }
  }
  double *quad_d = p->at_d, *gauss_d = quad_d + P, *stage_d = gauss_d + P, *nodes_d = stage_d + 4, *weights_d = nodes_d + rule_sz;
  const double p0 = fun_params ? fun_params[0] : 0.0, p1 = fun_params ? fun_params[1] : 0.0;
  const int lanes = quadrature_lanes(m + 1);
  const size_t lds = (size_t)3 * (m + 1) * lanes * 8;
  if (lds > 48 * 1024)
    HIP_TRY(hipFuncSetAttribute((const void *)k_quadrature_at, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  HIP_TRY(hipMemsetAsync(p->at_flags, 0, 2 * sizeof(int), st));
  const double residual_tol = std::sqrt((double)p->n) * p->run_rtol;  // (the stop rule of the run: lanczos.h:110)
  if (rule == 1 && m == deg) SLQ_TRY(flush_closing_tail(p));  // (the border of the Radau rule at m = deg is beta_deg; nothing else here reads the tail)
  PROFILED(p, SLQ_K_QUADRATURE,
           hipLaunchKernelGGL(k_quadrature_at, dim3((P + lanes - 1) / lanes), dim3(64), lds, st, p->st, m, rule, endpoint, residual_tol, lanes,
                              fun_id, p0, p1, quad_d, gauss_d, nodes_d, weights_d, p->at_flags));
  if (stage)
    hipLaunchKernelGGL(k_stage_reduce, dim3(1), dim3(kStageThreads), 0, st, P, (const double *)quad_d,
                       rule ? (const double *)gauss_d : (const double *)nullptr, stage_d);
  HIP_TRY(hipGetLastError());
  int flags[2] = {0, 0}, ring_bad = 0;
  HIP_TRY(hipMemcpyAsync(flags, p->at_flags, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&ring_bad, p->ring_fail_d, sizeof(int), hipMemcpyDeviceToHost, st));
  if (quad) HIP_TRY(hipMemcpyAsync(quad, quad_d, (size_t)P * 8, hipMemcpyDeviceToHost, st));
  if (nodes) HIP_TRY(hipMemcpyAsync(nodes, nodes_d, (size_t)P * kout * 8, hipMemcpyDeviceToHost, st));
  if (weights) HIP_TRY(hipMemcpyAsync(weights, weights_d, (size_t)P * kout * 8, hipMemcpyDeviceToHost, st));
  if (stage) HIP_TRY(hipMemcpyAsync(stage, stage_d, 4 * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  SLQ_TRY(ring_flag_status(ring_bad));
  if (flags[1]) return fail(SLQ_EINVAL, "slq_plan_quadrature_at: endpoint = %g is not below the smallest Ritz value of every probe", endpoint);
  if (flags[0]) return fail(SLQ_ENOTCONV, "tridiagonal QL did not converge for at least one probe");
  return SLQ_OK;
}

// test hook: mark a plan as holding `nstale` stale ring columns, as the drop-in slq_lanczos_* entry does for its own plan
// (tests/test_gpu_resume.py: such a plan is not resumable). Mark it back to 0 before any run.
extern "C" int slq_debug_plan_mark_stale(slq_plan *p, int nstale) {
  if (!p || nstale < 0) return fail(SLQ_EINVAL, "plan is NULL or nstale < 0");
  SLQ_TRY(need_lanczos(p, "slq_debug_plan_mark_stale"));
  p->nstale = nstale;
  return SLQ_OK;
}

extern "C" int slq_plan_get_basis(slq_plan *p, int probe, void *Q, int64_t ldq) {
  if (!p || !Q) return fail(SLQ_EINVAL, "plan/Q is NULL");
  SLQ_TRY(need_lanczos(p, "slq_plan_get_basis"));
  if (!p->keep_basis) return fail(SLQ_EINVAL, "plan was created without keep_basis");
  SLQ_TRY(need_finished_run(p, "slq_plan_get_basis"));
  if (probe < 0 || probe >= p->nprobes || ldq < p->n) return fail(SLQ_EINVAL, "bad probe index or ldq");
  HIP_TRY(hipSetDevice(p->ctx->device));
  hipStream_t st = p->ctx->stream;
  const int bp = p->bpad, deg = p->deg;
  std::vector<double> hn((size_t)(deg + 1) * bp), hscale((size_t)deg * bp, 0.0);
  HIP_TRY(hipMemcpyAsync(hn.data(), p->st.nu, hn.size() * 8, hipMemcpyDeviceToHost, st));
  SLQ_TRY(check_ring_flag(p));
  for (int t = 0; t < deg; ++t) {
    const double nu = hn[(size_t)t * bp + probe];
    hscale[(size_t)t * bp + probe] = nu > 0.0 ? 1.0 / nu : 0.0;
  }
  double *dscale = nullptr;
  HIP_TRY(hipMalloc((void **)&dscale, hscale.size() * 8));
  hipError_t e = hipMemcpyAsync(dscale, hscale.data(), hscale.size() * 8, hipMemcpyHostToDevice, st);
  int rc = e == hipSuccess ? SLQ_OK : fail(SLQ_EHIP, "scale upload: %s", hipGetErrorString(e));
  for (int t = 0; t < deg && rc == SLQ_OK; ++t)
    rc = panel_to_host(p, t, probe, 1, (char *)Q + (size_t)t * (size_t)ldq * p->esz, ldq, dscale + (size_t)t * bp);
  hipFree(dscale);
  return rc;
}

static int update_chunk_cols(const slq_plan *p) {
  const int V = p->dtype == SLQ_F64 ? 2 : 4;
  return std::min(192, (int)((150 * 1024 - sizeof(double) * kWaves * 64 * V) / ((size_t)p->PW * p->esz + sizeof(int))));  // (192: the update sweep's column masks)
}

// w(slot (j+1)%S) -= sum_{i<r} gamma[i] * W_{j-i}, gamma staged through LDS in chunks
// axpy: the first chunk also applies the three-term step's `w -= cB W_c` (the dots sweeps ran in mode 2 and stored nothing)
static int launch_reorth_update_range(slq_plan *p, int j, int istart, int r, bool axpy, int klass) {
  if (axpy && (istart != 0 || r < 1)) return fail(SLQ_EINVAL, "internal: the deferred axpy rides on column 0 of the first update chunk");
  hipStream_t st = p->ctx->stream;
  const int V = p->dtype == SLQ_F64 ? 2 : 4;
  const int kUpdChunk = update_chunk_cols(p);
  const dim3 gS(p->nblkS, p->NP);
  for (int i0 = istart; i0 < r; i0 += kUpdChunk) {
    const int rc = std::min(kUpdChunk, r - i0);
    const size_t lds = sizeof(double) * kWaves * 64 * V + (size_t)rc * p->PW * p->esz + (size_t)rc * sizeof(int);  // reduction scratch, gamma, per-column flags
    PROFILED(p, klass,
             DISPATCH(p->dtype, p->LPR,
                      (launch_reorth_update_kernel<F, L>(p, gS, lds, st, j, i0, rc, axpy && i0 == 0))));  // (axpy: column 0 of the chunk must be W_c)
  }
  return SLQ_OK;
}

static int launch_reorth_update(slq_plan *p, int j, int r, int istart, bool axpy, int klass) { return launch_reorth_update_range(p, j, istart, r, axpy, klass); }

// ---- two-pass f(A)v: the replay of a recompute plan -------------------------------------------------
static int launch_action_accumulate(slq_plan *p, int t0, int nc, bool init) {
  hipStream_t st = p->ctx->stream;
  const dim3 gS(p->nblkS, p->NP);
  PROFILED(p, SLQ_K_COMBINE,
           DISPATCH(p->dtype, p->LPR,
                    (k_action_accumulate<F, L><<<gS, dim3(kBlock), 0, st>>>(p->n, (const F *)p->ring, p->slot_stride, p->S, t0, nc,
                                                                          p->acc_coef + (size_t)t0 * p->bpad, p->bpad,
                                                                          (F *)slot_ptr(p, p->y_slot), init ? 1 : 0, p->acc_skip ? 1 : 0, p->sweep_cols_d + 2))));
  return SLQ_OK;
}

// the run's launch sequence again, in pieces of up to acc_cols steps, each followed by the accumulation of the columns it
// finished: after step j the ring holds W_{j+2-S} .. W_{j+1}, and S >= acc_cols + 1 keeps the piece's oldest column resident
static int enqueue_replay(slq_plan *p, double rtol) {
  int c0 = 0;
  for (int j = 0; j < p->deg; ++j) {
    if (j - c0 + 1 < p->acc_cols && j != p->deg - 1) continue;
    SLQ_TRY(enqueue_run(p, rtol, c0, j + 1));
    SLQ_TRY(launch_action_accumulate(p, c0, j + 1 - c0, c0 == 0));
    c0 = j + 1;
  }
  HIP_TRY(hipGetLastError());
  return SLQ_OK;
}

// pass 2: probes back from the stash, the state the original probe call left (init_from_probes with its arguments), the replay.
// Afterwards alpha, nu, steps hold the bits of pass 1 again and the output panel holds sum_t g_t W_t.
static int replay_action(slq_plan *p) {
  if (!p->stash_ready) return fail(SLQ_EINVAL, "internal: a recompute plan without stashed probes");
  SLQ_TRY(precond_check_fresh(p->op, "slq_plan_fun_action"));
  hipStream_t st = p->ctx->stream;
  const double rtol = p->run_rtol;
  HIP_TRY(hipMemcpyAsync(slot_ptr(p, 0), slot_ptr(p, p->v_slot), (size_t)p->slot_stride * p->esz, hipMemcpyDeviceToDevice, st));
  SLQ_TRY(init_from_probes(p, p->pdf_sphere, p->stash_unit, true));
  const bool graph_ok = p->sw.graph && !p->prof && p->op->kind != OP_CALLBACK && p->op->kind != OP_DEVICE_CALLBACK;
  int rc = SLQ_OK;
  if (!graph_ok) {
    rc = enqueue_replay(p, rtol);
  } else {
    const unsigned variant = graph_variant(p);  // (the replay has a cache of its own: replay_exec)
    if (p->replay_exec && (p->replay_rtol != rtol || p->replay_variant != variant)) {
      HIP_TRY(hipGraphExecDestroy(p->replay_exec));
      p->replay_exec = nullptr;
    }
    if (!p->replay_exec) {
      hipGraph_t graph = nullptr;
      HIP_TRY(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
      rc = enqueue_replay(p, rtol);
      hipError_t ce = hipStreamEndCapture(st, &graph);
      if (rc != SLQ_OK) {
        if (graph) hipGraphDestroy(graph);
      } else if (ce != hipSuccess) {
        rc = fail(SLQ_EHIP, "hipStreamEndCapture: %s", hipGetErrorString(ce));
      } else {
        ce = hipGraphInstantiate(&p->replay_exec, graph, nullptr, nullptr, 0);
        hipGraphDestroy(graph);
        if (ce != hipSuccess) {
          p->replay_exec = nullptr;
          rc = fail(SLQ_EHIP, "hipGraphInstantiate: %s", hipGetErrorString(ce));
        }
      }
      if (rc == SLQ_OK) {
        p->replay_rtol = rtol;
        p->replay_variant = variant;
        p->replay_xt_out = p->prev_xt;
      }
    }
    if (rc == SLQ_OK) {
      hipError_t le = hipGraphLaunch(p->replay_exec, st);
      if (le != hipSuccess) rc = fail(SLQ_EHIP, "hipGraphLaunch: %s", hipGetErrorString(le));
      p->prev_xt = p->replay_xt_out;
    }
  }
  p->probes_ready = false;
  if (rc != SLQ_OK) return rc;  // (ran stays false: the plan needs new probes and a run)
  p->ran = true;
  p->cur = p->deg;
  return SLQ_OK;
}

// Y = f(A) X on the device: result left in panel y_slot (kept basis: ring slot `deg`; recompute: behind the ring)
static int fun_action_device(slq_plan *p, int fun_id, const double *fun_params) {
  SLQ_TRY(need_lanczos(p, "slq_plan_fun_action / slq_diag_update"));
  if (p->basis_mode == 0) return fail(SLQ_EINVAL, "plan was created without keep_basis");
  const bool two_pass = p->basis_mode == 2;
  SLQ_TRY(need_finished_run(p, "slq_plan_fun_action / slq_diag_update"));
  if (fun_id < SLQ_FUN_IDENTITY || fun_id > SLQ_FUN_SOFTSIGN) return fail(SLQ_EINVAL, "Unknown function id %d.", fun_id);
  HIP_TRY(hipSetDevice(p->ctx->device));
  hipStream_t st = p->ctx->stream;
  const int deg = p->deg;
  const double p0 = fun_params ? fun_params[0] : 0.0, p1 = fun_params ? fun_params[1] : 0.0;
  // eigenvectors of every probe's T: in LDS up to deg = 141, beyond that in a global scratch (stays in L2)
  const size_t lds_onchip = ((size_t)2 * deg + (size_t)deg * (deg + 1)) * 8;
  const bool zg = lds_onchip > 160 * 1024;
  const size_t lds = zg ? (size_t)2 * deg * 8 : lds_onchip;
  double *zscr = nullptr;
  if (zg) HIP_TRY(hipMalloc((void **)&zscr, (size_t)p->nprobes * deg * (deg + 1) * 8));
  struct ScratchGuard { double *q; ~ScratchGuard() { if (q) hipFree(q); } } guard{zscr};
  if (lds > 48 * 1024)
    HIP_TRY(hipFuncSetAttribute((const void *)k_fun_coeffs<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  HIP_TRY(hipMemsetAsync(p->fail_d, 0, sizeof(int), st));
  // kept basis: gamma row deg-1-t = -g_t: the update kernel's "w -= gamma W" then accumulates +g_t W_t into a
  // zeroed slot while walking t = deg-1 .. 0. Recompute: row t = +g_t in a buffer of its own (st.gamma is live during the replay)
  double *coef = two_pass ? p->acc_coef : p->st.gamma;
  const double sign = two_pass ? 1.0 : -1.0;
  const int reverse_rows = two_pass ? 0 : 1;
  HIP_TRY(hipMemsetAsync(coef, 0, (size_t)deg * p->bpad * 8, st));
  if (zg) {
    PROFILED(p, SLQ_K_QUADRATURE,
             (k_fun_coeffs<true><<<dim3(p->nprobes), dim3(64), lds, st>>>(p->st, fun_id, p0, p1, sign, reverse_rows, coef, zscr, p->fail_d)));
  } else {
    PROFILED(p, SLQ_K_QUADRATURE,
             (k_fun_coeffs<false><<<dim3(p->nprobes), dim3(64), lds, st>>>(p->st, fun_id, p0, p1, sign, reverse_rows, coef, nullptr, p->fail_d)));
  }
  if (two_pass) {
    SLQ_TRY(replay_action(p));
  } else {
  // output accumulates in slot `deg` (the spare slot behind the basis; it held the last residual)
  HIP_TRY(hipMemsetAsync(slot_ptr(p, deg), 0, (size_t)p->slot_stride * p->esz, st));
  SLQ_TRY(launch_reorth_update(p, deg - 1, deg, 0, false, SLQ_K_COMBINE));  // (its own profile class: these bytes are not the recurrence's update sweep)
  }
  HIP_TRY(hipGetLastError());
  int bad = 0;
  HIP_TRY(hipMemcpyAsync(&bad, p->fail_d, sizeof(int), hipMemcpyDeviceToHost, st));
  SLQ_TRY(check_ring_flag(p));  // (synchronises)
  if (bad) return fail(SLQ_ENOTCONV, "tridiagonal QL did not converge for at least one probe");
  return SLQ_OK;
}

extern "C" int slq_plan_fun_action(slq_plan *p, int fun_id, const double *fun_params, void *Y, int64_t ldy) {
  if (!p || !Y) return fail(SLQ_EINVAL, "plan/Y is NULL");
  if (ldy < p->n) return fail(SLQ_EINVAL, "ldy < n");
  SLQ_TRY(fun_action_device(p, fun_id, fun_params));
  return panel_to_host(p, p->y_slot, 0, p->nprobes, Y, ldy, nullptr);
}

// ---- diagonal estimator state (device-resident) ----------------------------------------------------
struct slq_diag {
  slq_context *ctx;
  int64_t n, count;
  DevBuf buf;  // numer | denom | msum, n doubles each (in the operator's stored row order)
  const slq_operator *op;
  double *acc(int k) const { return buf.as<double>() + k * n; }
};

extern "C" int slq_diag_create(slq_context *ctx, int64_t n, slq_diag **out) {
  if (!ctx || !out || n <= 0) return fail(SLQ_EINVAL, "bad arguments");
  *out = nullptr;
  HIP_TRY(hipSetDevice(ctx->device));
  std::unique_ptr<slq_diag> d(new (std::nothrow) slq_diag{ctx, n, 0, {}, nullptr});
  if (!d) return fail(SLQ_ENOMEM, "host allocation failed");
  hipError_t e = d->buf.alloc((size_t)3 * n * 8);
  if (e == hipSuccess) e = hipMemsetAsync(d->buf.p, 0, (size_t)3 * n * 8, ctx->stream);
  if (e != hipSuccess) return fail(SLQ_ENOMEM, "diag accumulators: %s", hipGetErrorString(e));
  ctx_retain(ctx);
  *out = d.release();
  return SLQ_OK;
}

extern "C" int slq_diag_destroy(slq_diag *d) { return handle_destroy(d); }

extern "C" int slq_diag_update(slq_diag *d, slq_plan *p, int fun_id, const double *fun_params) {
  if (!d || !p) return fail(SLQ_EINVAL, "diag/plan is NULL");
  SLQ_TRY(need_lanczos(p, "slq_diag_update"));
  if (d->n != p->n || d->ctx != p->ctx) return fail(SLQ_EINVAL, "diag accumulator does not match the plan");
  if (d->op && d->op != p->op) return fail(SLQ_EINVAL, "diag accumulator was started with another operator");
  d->op = p->op;
  SLQ_TRY(fun_action_device(p, fun_id, fun_params));
  hipStream_t st = p->ctx->stream;
  // coefB is free after a run: reuse it for the per-probe scale of the stored probes
  k_probe_scale<<<dim3((p->bpad + 255) / 256), dim3(256), 0, st>>>(p->st, p->st.coefB);
  const dim3 g((p->n + 63) / 64);
  if (p->dtype == SLQ_F64)
    k_diag_accumulate<double><<<g, dim3(64), 0, st>>>(p->n, (const double *)slot_ptr(p, p->v_slot), (const double *)slot_ptr(p, p->y_slot),
                                                      p->PW, p->nprobes, p->st.coefB, d->acc(0), d->acc(1), d->acc(2));
  else
    k_diag_accumulate<float><<<g, dim3(64), 0, st>>>(p->n, (const float *)slot_ptr(p, p->v_slot), (const float *)slot_ptr(p, p->y_slot),
                                                     p->PW, p->nprobes, p->st.coefB, d->acc(0), d->acc(1), d->acc(2));
  HIP_TRY(hipGetLastError());
  d->count += p->nprobes;
  return SLQ_OK;
}

extern "C" int slq_diag_get(slq_diag *d, double *numer, double *denom, double *running_mean, int64_t *count) {
  if (!d) return fail(SLQ_EINVAL, "diag is NULL");
  HIP_TRY(hipSetDevice(d->ctx->device));
  hipStream_t st = d->ctx->stream;
  if (numer) HIP_TRY(hipMemcpyAsync(numer, d->acc(0), (size_t)d->n * 8, hipMemcpyDeviceToHost, st));
  if (denom) HIP_TRY(hipMemcpyAsync(denom, d->acc(1), (size_t)d->n * 8, hipMemcpyDeviceToHost, st));
  if (running_mean) HIP_TRY(hipMemcpyAsync(running_mean, d->acc(2), (size_t)d->n * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (running_mean && d->count > 0)
    for (int64_t i = 0; i < d->n; ++i) running_mean[i] /= (double)d->count;
  if (d->op && !d->op->perm_h.empty()) {  // stored row i is caller row perm[i]
    const std::vector<int32_t> &perm = d->op->perm_h;
    std::vector<double> tmp((size_t)d->n);
    for (double *arr : {numer, denom, running_mean}) {
      if (!arr) continue;
      for (int64_t i = 0; i < d->n; ++i) tmp[(size_t)perm[(size_t)i]] = arr[i];
      memcpy(arr, tmp.data(), (size_t)d->n * 8);
    }
  }
  if (count) *count = d->count;
  return SLQ_OK;
}


// ---- spectral density accumulator (device-resident; kernels in slq_density.hpp) -----------------------
struct slq_density {
  slq_context *ctx;
  int kind, G;
  double c0, c1;     // the kernel's constants (k_density_eval)
  int64_t count;     // probes folded so far
  DevBuf grid;       // G points or G + 1 edges
  DevBuf stat;       // mean | M2, G + 2 doubles each (columns G, G + 1: node mass below / above the grid), then the two flag words
  int *flags;        // [0] QL non-convergence, [1] ring bail-out word of a plan (behind stat's doubles)
  DevBuf phi;        // P x (G + 2) scratch of the per-probe values (density_scratch)
  std::vector<double> grid_h;  // SLQ_DENSITY_CHEBYSHEV: the grid on the host (checked against the bounds of every run folded in)
};

extern "C" int slq_density_create(slq_context *ctx, int kind, int ngrid, const double *grid, double bw, slq_density **out) {
  if (!ctx || !out || !grid) return fail(SLQ_EINVAL, "slq_density_create: NULL argument");
  *out = nullptr;
  if (kind < SLQ_DENSITY_GAUSSIAN || kind > SLQ_DENSITY_CHEBYSHEV) return fail(SLQ_EINVAL, "slq_density_create: unknown kind %d", kind);
  if (ngrid < 1) return fail(SLQ_EINVAL, "slq_density_create: ngrid = %d < 1", ngrid);
  const int npts = ngrid + (kind == SLQ_DENSITY_HISTOGRAM ? 1 : 0);
  for (int i = 0; i < npts; ++i) {
    if (!std::isfinite(grid[i])) return fail(SLQ_EINVAL, "slq_density_create: grid[%d] is not finite", i);
    if (i > 0 && !(grid[i] > grid[i - 1])) return fail(SLQ_EINVAL, "slq_density_create: the grid is not strictly increasing at %d", i);
  }
  const bool smooth = kind == SLQ_DENSITY_GAUSSIAN || kind == SLQ_DENSITY_LORENTZIAN;
  if (smooth && !(bw > 0.0 && std::isfinite(bw))) return fail(SLQ_EINVAL, "slq_density_create: bandwidth %g must be > 0", bw);
  HIP_TRY(hipSetDevice(ctx->device));
  std::unique_ptr<slq_density> d(new (std::nothrow) slq_density());
  if (!d) return fail(SLQ_ENOMEM, "host allocation failed");
  d->ctx = ctx; d->kind = kind; d->G = ngrid; d->count = 0;
  d->c0 = d->c1 = 0.0;
  if (kind == SLQ_DENSITY_GAUSSIAN) { d->c0 = 1.0 / (2.0 * bw * bw); d->c1 = 1.0 / (bw * std::sqrt(2.0 * M_PI)); }
  if (kind == SLQ_DENSITY_LORENTZIAN) { d->c0 = bw * bw; d->c1 = bw / M_PI; }
  d->flags = nullptr;
  if (kind == SLQ_DENSITY_CHEBYSHEV) d->grid_h.assign(grid, grid + ngrid);
  const size_t G2 = (size_t)ngrid + 2;
  hipError_t e = d->grid.alloc((size_t)npts * 8);
  if (e == hipSuccess) e = d->stat.alloc(2 * G2 * 8 + 2 * sizeof(int));
  if (e == hipSuccess) {
    d->flags = (int *)(d->stat.as<double>() + 2 * G2);
    e = hipMemcpyAsync(d->grid.p, grid, (size_t)npts * 8, hipMemcpyHostToDevice, ctx->stream);
  }
  if (e == hipSuccess) e = hipMemsetAsync(d->stat.p, 0, 2 * G2 * 8 + 2 * sizeof(int), ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // (the host grid may go away when this returns)
  if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? SLQ_ENOMEM : SLQ_EHIP, "density accumulators: %s", hipGetErrorString(e));
  ctx_retain(ctx);
  *out = d.release();
  return SLQ_OK;
}

extern "C" int slq_density_destroy(slq_density *d) { return handle_destroy(d); }

// the P x (G + 2) scratch of an update
static int density_scratch(slq_density *d, int P, hipStream_t st) {
  const size_t need = (size_t)P * (size_t)(d->G + 2) * 8;
  if (d->phi && d->phi.bytes() < need) HIP_TRY(hipStreamSynchronize(st));  // (the old scratch may still be read by the previous update)
  return devbuf_grow(d->phi, need, "density scratch");
}

// The density of the kernel polynomial method from the moments of a plan's last Chebyshev run (k_cheb_density_eval), folded by
// the same k_density_fold as every other kind. Synchronises once (the outside flags of the run decide whether it may be folded).
extern "C" int slq_density_update_moments(slq_density *d, slq_plan *p, int nweights, const double *damp) {
  if (!d || !p) return fail(SLQ_EINVAL, "slq_density_update_moments: density/plan is NULL");
  if (d->ctx != p->ctx) return fail(SLQ_EINVAL, "slq_density_update_moments: the plan belongs to another context");
  if (d->kind != SLQ_DENSITY_CHEBYSHEV) return fail(SLQ_EINVAL, "slq_density_update_moments: the accumulator's kind is %d, not SLQ_DENSITY_CHEBYSHEV", d->kind);
  SLQ_TRY(need_chebyshev(p, "slq_density_update_moments"));
  if (!p->cheb_ran) return fail(SLQ_EINVAL, "slq_density_update_moments: no completed run");
  const int K = 2 * p->deg + 1, P = p->nprobes, G2 = d->G + 2;
  if (nweights < 1 || nweights > K) return fail(SLQ_EINVAL, "slq_density_update_moments: nweights = %d must lie in [1, %d] (2 nsteps + 1 moments)", nweights, K);
  const double lo = p->cheb_c - p->cheb_h, hi = p->cheb_c + p->cheb_h;
  for (int g = 0; g < d->G; ++g)
    if (!(d->grid_h[g] > lo && d->grid_h[g] < hi))
      return fail(SLQ_EINVAL, "slq_density_update_moments: grid[%d] = %.17g is not strictly inside the bounds (%.17g, %.17g) of the run", g, d->grid_h[g], lo, hi);
  HIP_TRY(hipSetDevice(p->ctx->device));
  hipStream_t st = p->ctx->stream;
  if (damp) HIP_TRY(hipMemcpyAsync(p->cheb_coef, damp, (size_t)nweights * 8, hipMemcpyHostToDevice, st));  // (ahead of the synchronisation below: the caller's array may go away on return)
  std::vector<int> flags;
  int raised = 0;
  SLQ_TRY(cheb_flags(p, flags, &raised));
  if (raised) return cheb_outside_error(p, "slq_density_update_moments", raised);
  SLQ_TRY(density_scratch(d, P, st));
  const int nbg = (G2 + kDensEvalThreads - 1) / kDensEvalThreads;
  PROFILED(p, SLQ_K_QUADRATURE,
           hipLaunchKernelGGL(k_cheb_density_eval, dim3((unsigned)((int64_t)P * nbg)), dim3(kDensEvalThreads), 0, st, d->G, nweights, p->bpad,
                              (const double *)p->cheb_mu, damp ? (const double *)p->cheb_coef : (const double *)nullptr, d->grid.as<const double>(),
                              p->cheb_c, p->cheb_h, nbg, d->phi.as<double>()));
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_density_fold, dim3((G2 + 63) / 64), dim3(64 * kDensFoldWaves), 0, st, P, G2, d->count, d->phi.as<double>(), d->stat.as<double>(), d->stat.as<double>() + G2,
                     (const int *)nullptr, 0, (const int *)p->ring_fail_d, d->flags);
  HIP_TRY(hipGetLastError());
  d->count += P;
  return SLQ_OK;
}

extern "C" int slq_density_update(slq_density *d, slq_plan *p) {
  if (!d || !p) return fail(SLQ_EINVAL, "slq_density_update: density/plan is NULL");
  if (d->ctx != p->ctx) return fail(SLQ_EINVAL, "slq_density_update: the plan belongs to another context");
  SLQ_TRY(need_lanczos(p, "slq_density_update"));
  if (d->kind == SLQ_DENSITY_CHEBYSHEV) return fail(SLQ_EINVAL, "slq_density_update: a Chebyshev density is updated from moments (slq_density_update_moments)");
  SLQ_TRY(need_finished_run(p, "slq_density_update"));
  HIP_TRY(hipSetDevice(p->ctx->device));
  hipStream_t st = p->ctx->stream;
  const int P = p->nprobes, deg = p->deg, G2 = d->G + 2;
  SLQ_TRY(density_scratch(d, P, st));
  // the Gauss rule of this run: once per run, whoever asks first (slq_plan_quadrature or a density update)
  int *rule_fail = p->fail_d + 2;
  if (p->rule_src == 0) {
    const QuadShape q = quadrature_shape(deg, P);
    if (q.lds > 48 * 1024)
      HIP_TRY(hipFuncSetAttribute((const void *)k_quadrature, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIP_TRY(hipMemsetAsync(rule_fail, 0, sizeof(int), st));
    PROFILED(p, SLQ_K_QUADRATURE,
             hipLaunchKernelGGL(k_quadrature, dim3(q.grid), dim3(64), q.lds, st, p->st, q.lanes, (int)SLQ_FUN_NONE, 0.0, 0.0,
                                (double *)nullptr, p->nodes_d, p->weights_d, rule_fail));
    HIP_TRY(hipGetLastError());
    p->rule_src = 2;
  }
  const int nbg = (G2 + kDensEvalThreads - 1) / kDensEvalThreads;
  hipLaunchKernelGGL(k_density_eval, dim3((unsigned)((int64_t)P * nbg)), dim3(kDensEvalThreads), 0, st, d->kind, d->G, deg, p->nodes_d,
                     p->weights_d, p->st.vnorm2, d->grid.as<double>(), d->c0, d->c1, nbg, d->phi.as<double>());
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_density_fold, dim3((G2 + 63) / 64), dim3(64 * kDensFoldWaves), 0, st, P, G2, d->count, d->phi.as<double>(), d->stat.as<double>(),
                     d->stat.as<double>() + G2, (p->rule_src == 2 ? (const int *)rule_fail : nullptr), (p->rule_src == 1 ? p->rule_fail_h : 0),
                     (const int *)p->ring_fail_d, d->flags);
  HIP_TRY(hipGetLastError());
  d->count += P;
  return SLQ_OK;
}

extern "C" int slq_density_get(slq_density *d, double *mean, double *m2, double *outside, int64_t *count) {
  if (!d) return fail(SLQ_EINVAL, "slq_density_get: density is NULL");
  HIP_TRY(hipSetDevice(d->ctx->device));
  hipStream_t st = d->ctx->stream;
  const size_t G = (size_t)d->G, G2 = G + 2;
  std::vector<double> h(2 * G2);
  int flags[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(h.data(), d->stat.p, 2 * G2 * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(flags, d->flags, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (mean) memcpy(mean, h.data(), G * 8);
  if (m2) memcpy(m2, h.data() + G2, G * 8);
  if (outside) { outside[0] = h[G]; outside[1] = h[G + 1]; }
  if (count) *count = d->count;
  SLQ_TRY(ring_flag_status(flags[1]));
  if (flags[0]) return fail(SLQ_ENOTCONV, "tridiagonal QL did not converge for at least one probe of an update");
  return SLQ_OK;
}


// ---------------------------------------------------------------------------------------------------
// tall-skinny device matrices (xtrace / hutch++ dense algebra on the matrix cores)
// ---------------------------------------------------------------------------------------------------
struct slq_dmat {
  slq_context *ctx;
  int64_t n;
  int cols;
  double *d;    // column-major, ld = n: what every call site reads
  DevBuf own;   // the allocation behind d (slq_dmat_create); empty in a view of somebody else's columns (precond_trace_columns)
};

extern "C" int slq_dmat_create(slq_context *ctx, int64_t n, int cols, slq_dmat **out) {
  if (!ctx || !out || n <= 0 || cols <= 0) return fail(SLQ_EINVAL, "bad arguments");
  *out = nullptr;
  HIP_TRY(hipSetDevice(ctx->device));
  std::unique_ptr<slq_dmat> m(new (std::nothrow) slq_dmat{ctx, n, cols, nullptr, {}});
  if (!m) return fail(SLQ_ENOMEM, "host allocation failed");
  hipError_t e = m->own.alloc((size_t)n * cols * 8);
  m->d = m->own.as<double>();
  if (e == hipSuccess) e = hipMemsetAsync(m->d, 0, (size_t)n * cols * 8, ctx->stream);
  if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? SLQ_ENOMEM : SLQ_EHIP, "dmat: %s", hipGetErrorString(e));
  ctx_retain(ctx);
  *out = m.release();
  return SLQ_OK;
}

extern "C" int slq_dmat_destroy(slq_dmat *m) { return handle_destroy(m); }

static int dmat_range(const slq_dmat *m, int c0, int nc, const char *what) {
  if (!m) return fail(SLQ_EINVAL, "%s: matrix is NULL", what);
  if (c0 < 0 || nc <= 0 || c0 + nc > m->cols) return fail(SLQ_EINVAL, "%s: columns [%d, %d) outside [0, %d)", what, c0, c0 + nc, m->cols);
  return SLQ_OK;
}
// The operands of a product OUT[:, o0 : o0 + b] = (rout x rin operator) IN[:, i0 : i0 + b] on device matrices of the context ctx:
// the column ranges, the row counts, the context, no overlap inside one matrix; then the addresses of the first columns. The caller
// has checked b >= 1.
static int dmat_operands(slq_dmat *IN, int i0, slq_dmat *OUT, int o0, int b, int64_t rin, int64_t rout, const slq_context *ctx, const char *who, const double **in,
                         double **out) {
  char what[96];
  snprintf(what, sizeof what, "%s(IN)", who);
  SLQ_TRY(dmat_range(IN, i0, b, what));
  snprintf(what, sizeof what, "%s(OUT)", who);
  SLQ_TRY(dmat_range(OUT, o0, b, what));
  if (IN->n != rin) return fail(SLQ_EINVAL, "%s: IN has %lld rows, the product reads %lld", who, (long long)IN->n, (long long)rin);
  if (OUT->n != rout) return fail(SLQ_EINVAL, "%s: OUT has %lld rows, the product writes %lld", who, (long long)OUT->n, (long long)rout);
  if (IN->ctx != ctx || OUT->ctx != ctx) return fail(SLQ_EINVAL, "%s: a matrix belongs to another context", who);
  if (IN == OUT && i0 < o0 + b && o0 < i0 + b) return fail(SLQ_EINVAL, "%s: the columns [%d, %d) of IN and [%d, %d) of OUT overlap in one matrix", who, i0, i0 + b, o0, o0 + b);
  *in = IN->d + (size_t)i0 * IN->n, *out = OUT->d + (size_t)o0 * OUT->n;
  return SLQ_OK;
}
// Y = (operator) X for host panels (X rin x b, ldx apart; Y rout x b, ldy apart; elements of es bytes) through the two staging
// buffers of the object: both grown on demand, a pitched copy in, run(in, ld_in, out, ld_out) enqueues the device product on the
// context's stream, a pitched copy out, and the one synchronisation. The caller has checked X, Y, b and the leading dimensions.
template <typename Run>
static int staged_panel_product(slq_context *ctx, size_t es, DevBuf &stage_in, DevBuf &stage_out, const void *X, int64_t ldx, int64_t rin, void *Y, int64_t ldy,
                                int64_t rout, int b, const char *who, Run run) {
  HIP_TRY(hipSetDevice(ctx->device));
  SLQ_TRY(devbuf_grow(stage_in, (size_t)rin * b * es, who, "staging buffer"));
  SLQ_TRY(devbuf_grow(stage_out, (size_t)rout * b * es, who, "staging buffer"));
  HIP_TRY(hipMemcpy2DAsync(stage_in.p, (size_t)rin * es, X, (size_t)ldx * es, (size_t)rin * es, (size_t)b, hipMemcpyHostToDevice, ctx->stream));
  SLQ_TRY(run(stage_in.p, rin, stage_out.p, rout));
  HIP_TRY(hipMemcpy2DAsync(Y, (size_t)ldy * es, stage_out.p, (size_t)rout * es, (size_t)rout * es, (size_t)b, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return SLQ_OK;
}

extern "C" int slq_dmat_set(slq_dmat *m, int c0, int nc, const double *host, int64_t ld) {
  SLQ_TRY(dmat_range(m, c0, nc, "slq_dmat_set"));
  if (!host || ld < m->n) return fail(SLQ_EINVAL, "bad host array");
  HIP_TRY(hipSetDevice(m->ctx->device));
  HIP_TRY(hipMemcpy2DAsync(m->d + (size_t)c0 * m->n, (size_t)m->n * 8, host, (size_t)ld * 8, (size_t)m->n * 8, (size_t)nc,
                           hipMemcpyHostToDevice, m->ctx->stream));
  HIP_TRY(hipStreamSynchronize(m->ctx->stream));
  return SLQ_OK;
}

extern "C" int slq_dmat_get(slq_dmat *m, int c0, int nc, double *host, int64_t ld) {
  SLQ_TRY(dmat_range(m, c0, nc, "slq_dmat_get"));
  if (!host || ld < m->n) return fail(SLQ_EINVAL, "bad host array");
  HIP_TRY(hipSetDevice(m->ctx->device));
  HIP_TRY(hipMemcpy2DAsync(host, (size_t)ld * 8, m->d + (size_t)c0 * m->n, (size_t)m->n * 8, (size_t)m->n * 8, (size_t)nc,
                           hipMemcpyDeviceToHost, m->ctx->stream));
  HIP_TRY(hipStreamSynchronize(m->ctx->stream));
  return SLQ_OK;
}

extern "C" int slq_dmat_ptr(slq_dmat *m, int c0, void **dptr) {
  SLQ_TRY(dmat_range(m, c0, 1, "slq_dmat_ptr"));
  if (!dptr) return fail(SLQ_EINVAL, "dptr is NULL");
  *dptr = m->d + (size_t)c0 * m->n;
  return SLQ_OK;
}

extern "C" int slq_dmat_generate(slq_dmat *m, int c0, int nc, int pdf, uint64_t seed, uint64_t probe_offset) {
  SLQ_TRY(dmat_range(m, c0, nc, "slq_dmat_generate"));
  if (pdf < 0 || pdf > 2) return fail(SLQ_EINVAL, "Invalid distribution id %d supplied.", pdf);
  HIP_TRY(hipSetDevice(m->ctx->device));
  hipStream_t st = m->ctx->stream;
  double *x = m->d + (size_t)c0 * m->n;
  k_gen_cols<<<dim3((unsigned)((m->n + 255) / 256)), dim3(256), 0, st>>>(m->n, x, nc, pdf == SLQ_PDF_RADEMACHER ? 0 : 1, seed, probe_offset);
  if (pdf == SLQ_PDF_SPHERE) k_scale_cols_sphere<<<dim3(nc), dim3(256), 0, st>>>(m->n, x);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  return SLQ_OK;
}

extern "C" int slq_dmat_copy(slq_dmat *dst, int d0, slq_dmat *src, int s0, int nc) {
  SLQ_TRY(dmat_range(dst, d0, nc, "slq_dmat_copy(dst)"));
  SLQ_TRY(dmat_range(src, s0, nc, "slq_dmat_copy(src)"));
  if (dst->n != src->n || dst->ctx != src->ctx) return fail(SLQ_EINVAL, "mismatched operands");
  HIP_TRY(hipSetDevice(dst->ctx->device));
  HIP_TRY(hipMemcpyAsync(dst->d + (size_t)d0 * dst->n, src->d + (size_t)s0 * src->n, (size_t)nc * dst->n * 8,
                         hipMemcpyDeviceToDevice, dst->ctx->stream));
  HIP_TRY(hipStreamSynchronize(dst->ctx->stream));
  return SLQ_OK;
}

// dst[dr0 : dr0 + nrows, d0 : d0 + nc] = src[sr0 : sr0 + nrows, s0 : s0 + nc]: a block of rows of some columns, between matrices
// of different heights - what a row-sharded sketch (primate_amd.distributed) takes out of / puts into full columns.
extern "C" int slq_dmat_copy_rows(slq_dmat *dst, int d0, int64_t dr0, slq_dmat *src, int s0, int64_t sr0, int64_t nrows, int nc) {
  SLQ_TRY(dmat_range(dst, d0, nc, "slq_dmat_copy_rows(dst)"));
  SLQ_TRY(dmat_range(src, s0, nc, "slq_dmat_copy_rows(src)"));
  if (dst->ctx != src->ctx) return fail(SLQ_EINVAL, "mismatched operands");
  if (nrows == 0) return SLQ_OK;  // (an empty shard - more ranks than rows - copies nothing, wherever it nominally starts)
  if (nrows < 0 || dr0 < 0 || sr0 < 0 || dr0 + nrows > dst->n || sr0 + nrows > src->n) return fail(SLQ_EINVAL, "row range outside the matrix");
  HIP_TRY(hipSetDevice(dst->ctx->device));
  HIP_TRY(hipMemcpy2DAsync(dst->d + (size_t)d0 * dst->n + dr0, (size_t)dst->n * 8, src->d + (size_t)s0 * src->n + sr0, (size_t)src->n * 8,
                           (size_t)nrows * 8, (size_t)nc, hipMemcpyDeviceToDevice, dst->ctx->stream));
  HIP_TRY(hipStreamSynchronize(dst->ctx->stream));
  return SLQ_OK;
}

extern "C" int slq_dmat_gemm_tn(slq_dmat *A, int a0, int ma, slq_dmat *B, int b0, int mb, double *C_host) {
  SLQ_TRY(dmat_range(A, a0, ma, "slq_dmat_gemm_tn(A)"));
  SLQ_TRY(dmat_range(B, b0, mb, "slq_dmat_gemm_tn(B)"));
  if (!C_host || A->n != B->n || A->ctx != B->ctx) return fail(SLQ_EINVAL, "mismatched operands");
  slq_context *ctx = A->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int n = (int)A->n;
  const int tiles = ((ma + 16 * kTnA - 1) / (16 * kTnA)) * ((mb + 16 * kTnB - 1) / (16 * kTnB));
  // enough single-wave workgroups to fill the chip: ~16 per CU
  int nslab = std::max(1, std::min((n + 1023) / 1024, (ctx->num_cus * 16 + tiles - 1) / tiles));
  int slab_rows = ((n + nslab - 1) / nslab + 15) / 16 * 16;
  nslab = (n + slab_rows - 1) / slab_rows;
  const size_t cnt = (size_t)ma * mb;
  double *buf = nullptr;
  HIP_TRY(hipMalloc((void **)&buf, ((size_t)nslab + 1) * cnt * 8));
  k_gemm_tn<<<dim3(tiles, nslab), dim3(64), 0, st>>>(n, A->d + (size_t)a0 * n, (int64_t)n, B->d + (size_t)b0 * n, (int64_t)n, ma, mb,
                                                    slab_rows, buf);
  k_sum_slabs<<<dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st>>>(buf, nslab, (int64_t)cnt, buf + (size_t)nslab * cnt);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(C_host, buf + (size_t)nslab * cnt, cnt * 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  hipFree(buf);
  if (e != hipSuccess) return fail(SLQ_EHIP, "slq_dmat_gemm_tn: %s", hipGetErrorString(e));
  return SLQ_OK;
}

extern "C" int slq_dmat_gemm_nn(slq_dmat *OUT, int o0, slq_dmat *A, int a0, int ma, const double *C_host, int mb,
                                double alpha, double beta) {
  SLQ_TRY(dmat_range(OUT, o0, mb, "slq_dmat_gemm_nn(OUT)"));
  SLQ_TRY(dmat_range(A, a0, ma, "slq_dmat_gemm_nn(A)"));
  if (!C_host || A->n != OUT->n || A->ctx != OUT->ctx) return fail(SLQ_EINVAL, "mismatched operands");
  if (A == OUT && !(o0 + mb <= a0 || a0 + ma <= o0)) return fail(SLQ_EINVAL, "output columns overlap the input columns");
  slq_context *ctx = A->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int n = (int)A->n;
  double *dC = nullptr;
  HIP_TRY(hipMalloc((void **)&dC, (size_t)ma * mb * 8));
  hipError_t e = hipMemcpyAsync(dC, C_host, (size_t)ma * mb * 8, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    k_gemm_nn<<<dim3((n + 15) / 16, (mb + 16 * kNnB - 1) / (16 * kNnB)), dim3(64), 0, st>>>(
        n, OUT->d + (size_t)o0 * n, (int64_t)n, A->d + (size_t)a0 * n, (int64_t)n, ma, dC, mb, alpha, beta);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  hipFree(dC);
  if (e != hipSuccess) return fail(SLQ_EHIP, "slq_dmat_gemm_nn: %s", hipGetErrorString(e));
  return SLQ_OK;
}

// f(A) X for the probes of a completed keep_basis run, written to OUT[:, o0 : o0 + nprobes] (fp64 plans)
extern "C" int slq_plan_fun_action_dmat(slq_plan *p, int fun_id, const double *fun_params, slq_dmat *OUT, int o0) {
  if (!p) return fail(SLQ_EINVAL, "plan is NULL");
  SLQ_TRY(dmat_range(OUT, o0, p->nprobes, "slq_plan_fun_action_dmat"));
  if (p->dtype != SLQ_F64 || OUT->n != p->n || OUT->ctx != p->ctx) return fail(SLQ_EINVAL, "plan and matrix do not match (fp64, same n, same context)");
  SLQ_TRY(fun_action_device(p, fun_id, fun_params));
  hipStream_t st = p->ctx->stream;
  dim3 g((p->n + 63) / 64, (p->nprobes + 63) / 64);
  hipLaunchKernelGGL(k_panel_to_cols<double>, g, dim3(256), 0, st, p->n, (const double *)slot_ptr(p, p->y_slot), 0, p->nprobes,
                     OUT->d + (size_t)o0 * p->n, p->PW, (const double *)nullptr, p->op->perm_d.as<int32_t>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  return SLQ_OK;
}

// the Chebyshev action of an action plan, written to OUT[:, o0 : o0 + nprobes] (fp64 plans)
extern "C" int slq_plan_chebyshev_action_dmat(slq_plan *p, double center, double halfwidth, double outside_tol, int ncoef, const double *coef,
                                              slq_dmat *OUT, int o0) {
  if (!p) return fail(SLQ_EINVAL, "plan is NULL");
  SLQ_TRY(dmat_range(OUT, o0, p->nprobes, "slq_plan_chebyshev_action_dmat"));
  if (p->dtype != SLQ_F64 || OUT->n != p->n || OUT->ctx != p->ctx) return fail(SLQ_EINVAL, "plan and matrix do not match (fp64, same n, same context)");
  SLQ_TRY(cheb_action_device(p, "slq_plan_chebyshev_action_dmat", center, halfwidth, outside_tol, ncoef, coef));
  hipStream_t st = p->ctx->stream;
  dim3 g((p->n + 63) / 64, (p->nprobes + 63) / 64);
  hipLaunchKernelGGL(k_panel_to_cols<double>, g, dim3(256), 0, st, p->n, (const double *)slot_ptr(p, p->y_slot), 0, p->nprobes,
                     OUT->d + (size_t)o0 * p->n, p->PW, (const double *)nullptr, p->op->perm_d.as<int32_t>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  return SLQ_OK;
}

extern "C" int slq_plan_get_probes_dmat(slq_plan *p, slq_dmat *OUT, int o0) {
  if (!p) return fail(SLQ_EINVAL, "plan is NULL");
  if (!p->probes_ready) return fail(SLQ_EINVAL, "no probes set, or they were consumed by a run");
  SLQ_TRY(dmat_range(OUT, o0, p->nprobes, "slq_plan_get_probes_dmat"));
  if (p->dtype != SLQ_F64 || OUT->n != p->n || OUT->ctx != p->ctx) return fail(SLQ_EINVAL, "plan and matrix do not match (fp64, same n, same context)");
  HIP_TRY(hipSetDevice(p->ctx->device));
  hipStream_t st = p->ctx->stream;
  // the probes as the estimators see them: sphere probes are stored as the normal draw g and used as
  // sqrt(n) g / ||g|| (k_fin_init), so the copy carries that scale (coefB is free until the run starts)
  k_probe_scale<<<dim3((p->bpad + 255) / 256), dim3(256), 0, st>>>(p->st, p->st.coefB);
  dim3 g((p->n + 63) / 64, (p->nprobes + 63) / 64);
  hipLaunchKernelGGL(k_panel_to_cols<double>, g, dim3(256), 0, st, p->n, (const double *)slot_ptr(p, 0), 0, p->nprobes,
                     OUT->d + (size_t)o0 * p->n, p->PW, (const double *)p->st.coefB, p->op->perm_d.as<int32_t>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  return SLQ_OK;
}

// ---- sampled dense-dense product on a CSR pattern (device-resident values; schedule and kernel in slq_sddmm.hpp) -------------
struct slq_sddmm {
  slq_context *ctx;
  int64_t n, nnz, count, nitems, grid;
  DevBuf rowptr, colind;  // int32: the caller's pattern as validated on the host (never the caller's own device arrays)
  DevBuf items;           // SddmmItem
  DevBuf vals;            // nnz doubles
};

static int sddmm_create_body(slq_context *ctx, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colind, slq_sddmm **out, const char *what) {
  const int64_t bad = sddmm_first_bad_row(n, nnz, rowptr, colind);
  if (bad >= 0)
    return fail(SLQ_EINVAL, "%s: not a CSR pattern over %lld rows at row %lld (rowptr[0] == 0, rowptr non-decreasing, rowptr[n] == nnz = %lld, 0 <= colind < n)",
                what, (long long)n, (long long)bad, (long long)nnz);
  HIP_TRY(hipSetDevice(ctx->device));
  if (ctx->dead) return fail(SLQ_EINVAL, "%s: the context has been destroyed", what);
  const SddmmSchedule S = sddmm_schedule(n, rowptr);
  std::unique_ptr<slq_sddmm> s(new (std::nothrow) slq_sddmm{ctx, n, nnz, 0, (int64_t)S.items.size(), S.grid, {}, {}, {}, {}});
  if (!s) return fail(SLQ_ENOMEM, "host allocation failed");
  hipStream_t st = ctx->stream;
  hipError_t e = s->rowptr.alloc(((size_t)n + 1) * 4);
  if (e == hipSuccess) e = s->colind.alloc(std::max<size_t>((size_t)nnz, 1) * 4);
  if (e == hipSuccess) e = s->vals.alloc(std::max<size_t>((size_t)nnz, 1) * 8);
  if (e == hipSuccess) e = s->items.alloc(std::max<size_t>(S.items.size(), 1) * sizeof(SddmmItem));
  if (e == hipSuccess) e = hipMemcpyAsync(s->rowptr.p, rowptr, ((size_t)n + 1) * 4, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && nnz) e = hipMemcpyAsync(s->colind.p, colind, (size_t)nnz * 4, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && !S.items.empty()) e = hipMemcpyAsync(s->items.p, S.items.data(), S.items.size() * sizeof(SddmmItem), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync(s->vals.p, 0, std::max<size_t>((size_t)nnz, 1) * 8, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);  // (the host arrays are the caller's, or locals of this call)
  if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? SLQ_ENOMEM : SLQ_EHIP, "%s: %s", what, hipGetErrorString(e));
  ctx_retain(ctx);
  *out = s.release();
  return SLQ_OK;
}

static int sddmm_shape_check(slq_context *ctx, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colind, slq_sddmm **out, const char *what) {
  if (!ctx || !out) return fail(SLQ_EINVAL, "%s: ctx/out is NULL", what);
  *out = nullptr;
  if (n <= 0 || n >= (int64_t)1 << 31 || nnz < 0 || nnz >= (int64_t)1 << 31) return fail(SLQ_EINVAL, "%s: pattern shape out of range for int32 indices", what);
  if (!rowptr || (nnz > 0 && !colind)) return fail(SLQ_EINVAL, "%s: pattern arrays are NULL", what);
  return SLQ_OK;
}

extern "C" int slq_sddmm_create(slq_context *ctx, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colind, slq_sddmm **out) {
  SLQ_TRY(sddmm_shape_check(ctx, n, nnz, rowptr, colind, out, "slq_sddmm_create"));
  try {
    return sddmm_create_body(ctx, n, nnz, rowptr, colind, out, "slq_sddmm_create");
  } catch (const std::bad_alloc &) {
    return fail(SLQ_ENOMEM, "slq_sddmm_create: host allocation failed");
  }
}

extern "C" int slq_sddmm_create_device(slq_context *ctx, int64_t n, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_colind, slq_sddmm **out) {
  SLQ_TRY(sddmm_shape_check(ctx, n, nnz, d_rowptr, d_colind, out, "slq_sddmm_create_device"));
  try {
    // the index arrays come back once (4 bytes per nonzero); what the kernel reads is the validated copy, not the caller's arrays
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<int32_t> rp((size_t)n + 1), ci((size_t)nnz);
    HIP_TRY(hipMemcpy(rp.data(), d_rowptr, ((size_t)n + 1) * 4, hipMemcpyDeviceToHost));
    if (nnz) HIP_TRY(hipMemcpy(ci.data(), d_colind, (size_t)nnz * 4, hipMemcpyDeviceToHost));
    return sddmm_create_body(ctx, n, nnz, rp.data(), ci.data(), out, "slq_sddmm_create_device");
  } catch (const std::bad_alloc &) {
    return fail(SLQ_ENOMEM, "slq_sddmm_create_device: host allocation failed");
  }
}

extern "C" int slq_sddmm_destroy(slq_sddmm *s) { return handle_destroy(s); }

extern "C" int slq_sddmm_update(slq_sddmm *s, slq_dmat *W, int w0, slq_dmat *Z, int z0, int m, double alpha, double beta, int symmetric) {
  if (!s) return fail(SLQ_EINVAL, "slq_sddmm_update: accumulator is NULL");
  SLQ_TRY(dmat_range(W, w0, m, "slq_sddmm_update(W)"));
  SLQ_TRY(dmat_range(Z, z0, m, "slq_sddmm_update(Z)"));
  if (W->n != s->n || Z->n != s->n)
    return fail(SLQ_EINVAL, "slq_sddmm_update: the pattern has %lld rows, W %lld, Z %lld", (long long)s->n, (long long)W->n, (long long)Z->n);
  if (W->ctx != s->ctx || Z->ctx != s->ctx) return fail(SLQ_EINVAL, "slq_sddmm_update: a matrix belongs to another context");
  if (!std::isfinite(alpha) || !std::isfinite(beta)) return fail(SLQ_EINVAL, "slq_sddmm_update: alpha = %g, beta = %g must be finite", alpha, beta);
  HIP_TRY(hipSetDevice(s->ctx->device));
  if (s->nitems > 0) {
    const double *w = W->d + (size_t)w0 * s->n, *z = Z->d + (size_t)z0 * s->n;
    const dim3 g((unsigned)s->grid), b(64 * kSddmmWaves);
    if (symmetric)
      k_sddmm<true><<<g, b, 0, s->ctx->stream>>>(s->nitems, s->items.as<SddmmItem>(), s->rowptr.as<int32_t>(), s->colind.as<int32_t>(), s->n, w, z, m, 0.5 * alpha, beta, s->vals.as<double>());
    else
      k_sddmm<false><<<g, b, 0, s->ctx->stream>>>(s->nitems, s->items.as<SddmmItem>(), s->rowptr.as<int32_t>(), s->colind.as<int32_t>(), s->n, w, z, m, alpha, beta, s->vals.as<double>());
    HIP_TRY(hipGetLastError());
  }
  s->count += m;
  return SLQ_OK;
}

extern "C" int slq_sddmm_get(slq_sddmm *s, double *vals, int64_t *count) {
  if (!s) return fail(SLQ_EINVAL, "slq_sddmm_get: accumulator is NULL");
  HIP_TRY(hipSetDevice(s->ctx->device));
  if (vals && s->nnz) HIP_TRY(hipMemcpyAsync(vals, s->vals.p, (size_t)s->nnz * 8, hipMemcpyDeviceToHost, s->ctx->stream));
  HIP_TRY(hipStreamSynchronize(s->ctx->stream));
  if (count) *count = s->count;
  return SLQ_OK;
}

extern "C" int slq_sddmm_ptr(slq_sddmm *s, void **d_vals) {
  if (!s || !d_vals) return fail(SLQ_EINVAL, "slq_sddmm_ptr: NULL argument");
  *d_vals = s->vals.p;
  return SLQ_OK;
}

extern "C" int slq_sddmm_reset(slq_sddmm *s) {
  if (!s) return fail(SLQ_EINVAL, "slq_sddmm_reset: accumulator is NULL");
  HIP_TRY(hipSetDevice(s->ctx->device));
  HIP_TRY(hipMemsetAsync(s->vals.p, 0, std::max<size_t>((size_t)s->nnz, 1) * 8, s->ctx->stream));
  s->count = 0;
  return SLQ_OK;
}

extern "C" int slq_debug_sddmm_schedule(int64_t n, const int32_t *rowptr, int32_t *row0, int32_t *nrows, int32_t *kind, int64_t *e0, int64_t *e1, int64_t cap,
                                        int64_t *nitems, int64_t *info) {
  if (!rowptr || !nitems || n <= 0 || n >= (int64_t)1 << 31 || cap < 0) return fail(SLQ_EINVAL, "slq_debug_sddmm_schedule: rowptr, nitems, 0 < n < 2^31, cap >= 0");
  if (rowptr[0] != 0) return fail(SLQ_EINVAL, "slq_debug_sddmm_schedule: rowptr[0] = %d, not 0", rowptr[0]);
  for (int64_t i = 0; i < n; ++i)
    if (rowptr[i + 1] < rowptr[i]) return fail(SLQ_EINVAL, "slq_debug_sddmm_schedule: rowptr is not non-decreasing at row %lld", (long long)i);
  try {
    const SddmmSchedule S = sddmm_schedule(n, rowptr);
    *nitems = (int64_t)S.items.size();
    for (int64_t i = 0; i < std::min<int64_t>(cap, *nitems); ++i) {
      const SddmmItem &it = S.items[(size_t)i];
      int64_t a, b;
      sddmm_item_range(it, rowptr, &a, &b);
      if (row0) row0[i] = it.row0;
      if (nrows) nrows[i] = it.nrows ? it.nrows : 1;
      if (kind) kind[i] = it.nrows ? 0 : 1;
      if (e0) e0[i] = a;
      if (e1) e1[i] = b;
    }
    if (info) { info[0] = S.grid; info[1] = S.nlong; info[2] = kSddmmLongRow; info[3] = kSddmmWaves; }
  } catch (const std::bad_alloc &) {
    return fail(SLQ_ENOMEM, "slq_debug_sddmm_schedule: host allocation failed");
  }
  return SLQ_OK;
}

// ---- hyperparameter gradients of the kernel operator (schedule and kernels in slq_kernelgrad.hpp) -------------
struct slq_kernel_grad {
  slq_context *ctx;
  slq_operator *op;  // not owned: read at every update (its z, norms and scalars as they are then)
  int64_t n, count, nparts;
  int d, dpad;
  DevBuf vals;  // d + 2 doubles
  DevBuf part;  // nparts x (dpad + 2) doubles: one partial per workgroup of a launch
};
static const char *op_kind_name(int kind) {
  switch (kind) {
    case OP_CSR: return "csr";
    case OP_DENSE: return "dense";
    case OP_CALLBACK: return "callback";
    case OP_DEVICE_CALLBACK: return "device_callback";
    case OP_GRAM: return "gram";
    case OP_KERNEL: return "kernel";
    case OP_KERNEL_PRECOND: return "kernel_precond";
    case OP_TOEPLITZ: return "toeplitz";
    default: return "?";
  }
}
// "A kernel operator this object may be built on", for the creates of the side objects: a kernel operator (of a preconditioned one
// its base: hint_base says so), unscaled where the object is not built for a diagonal scale, fp64 where the object is, on ctx, and
// ctx alive.
static int kernel_base_check(slq_context *ctx, const slq_operator *op, const char *who, bool f64_only, bool refuse_scaled, bool hint_base) {
  if (hint_base && op->kind == OP_KERNEL_PRECOND)
    return fail(SLQ_EINVAL, "%s: the operator is of kind 'kernel_precond': the object belongs to the kernel operator it was built on (pass its base)", who);
  if (op->kind != OP_KERNEL) return fail(SLQ_EINVAL, "%s: the operator is of kind '%s', not a kernel operator (slq_kernel_create)", who, op_kind_name(op->kind));
  if (refuse_scaled) SLQ_TRY(kernel_refuse_scaled(op, who));
  if (f64_only && op->dtype != SLQ_F64) return fail(SLQ_EINVAL, "%s: the operator's dtype is fp32: the object is fp64 only (the device matrices are fp64)", who);
  if (op->ctx != ctx) return fail(SLQ_EINVAL, "%s: the operator belongs to another context", who);
  if (ctx->dead) return fail(SLQ_EINVAL, "%s: the context has been destroyed", who);
  return SLQ_OK;
}

extern "C" int slq_kernel_grad_create(slq_context *ctx, slq_operator *op, slq_kernel_grad **out) {
  if (!ctx || !op || !out) return fail(SLQ_EINVAL, "slq_kernel_grad_create: ctx/op/out is NULL");
  *out = nullptr;
  SLQ_TRY(kernel_base_check(ctx, op, "slq_kernel_grad_create", true, true, false));
  HIP_TRY(hipSetDevice(ctx->device));
  const KernelGradSchedule S = kernel_grad_schedule(op->n, 1, ctx->num_cus);
  std::unique_ptr<slq_kernel_grad> g(new (std::nothrow) slq_kernel_grad{ctx, op, op->n, 0, S.nparts(), op->k_pts.d, op->k_pts.dpad, {}, {}});
  if (!g) return fail(SLQ_ENOMEM, "host allocation failed");
  hipError_t e = g->vals.alloc((size_t)(g->d + 2) * 8);
  if (e == hipSuccess) e = g->part.alloc((size_t)g->nparts * (size_t)(g->dpad + 2) * 8);
  if (e == hipSuccess) e = hipMemsetAsync(g->vals.p, 0, (size_t)(g->d + 2) * 8, ctx->stream);
  if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? SLQ_ENOMEM : SLQ_EHIP, "slq_kernel_grad_create: %s", hipGetErrorString(e));
  ctx_retain(ctx);
  *out = g.release();
  return SLQ_OK;
}

extern "C" int slq_kernel_grad_destroy(slq_kernel_grad *g) { return handle_destroy(g); }

extern "C" int slq_kernel_grad_update(slq_kernel_grad *g, slq_dmat *Z, int z0, slq_dmat *W, int w0, int m, double alpha, double beta) {
  if (!g) return fail(SLQ_EINVAL, "slq_kernel_grad_update: accumulator is NULL");
  if (m < 1) return fail(SLQ_EINVAL, "slq_kernel_grad_update: m = %d columns (m >= 1)", m);
  SLQ_TRY(dmat_range(Z, z0, m, "slq_kernel_grad_update(Z)"));
  SLQ_TRY(dmat_range(W, w0, m, "slq_kernel_grad_update(W)"));
  if (W->n != g->n || Z->n != g->n)
    return fail(SLQ_EINVAL, "slq_kernel_grad_update: the operator has %lld points, Z %lld rows, W %lld", (long long)g->n, (long long)Z->n, (long long)W->n);
  if (W->ctx != g->ctx || Z->ctx != g->ctx) return fail(SLQ_EINVAL, "slq_kernel_grad_update: a matrix belongs to another context");
  if (!std::isfinite(alpha) || !std::isfinite(beta)) return fail(SLQ_EINVAL, "slq_kernel_grad_update: alpha = %g, beta = %g must be finite", alpha, beta);
  SLQ_TRY(kernel_refuse_scaled(g->op, "slq_kernel_grad_update"));
  HIP_TRY(hipSetDevice(g->ctx->device));
  const slq_operator *op = g->op;
  const KernelGradSchedule S = kernel_grad_schedule(g->n, m, g->ctx->num_cus);
  if (S.nparts() != g->nparts) return fail(SLQ_EINVAL, "slq_kernel_grad_update: the schedule has %lld workgroups, the accumulator room for %lld", (long long)S.nparts(), (long long)g->nparts);
  KernelGradScale sc;
  for (int k = 0; k < kKernelMaxDim; ++k) sc.ls[k] = op->k_scale->ls[k];
  hipStream_t st = g->ctx->stream;
  for (int ch = 0; ch < S.ncol_chunks; ++ch) {
    const int c0 = ch * S.chunk_cols, mc = std::min(S.chunk_cols, m - c0);
    const KernelGradArgs a{(int)g->n, (int)op->k_pts.npad, g->dpad / 4, (const double *)op->k_pts.zt, (const double *)op->k_pts.nrm,
                           Z->d + (size_t)(z0 + c0) * g->n, W->d + (size_t)(w0 + c0) * g->n, mc, S.tiles_per_slab, g->part.as<double>()};
    if (!kernel_grad_launch(op->k_profile, S, a, st)) return fail(SLQ_EINVAL, "slq_kernel_grad_update: no kernel for profile %d", op->k_profile);
    HIP_TRY(hipGetLastError());
    // (the chunks run one after the other on the stream: each reads the partials of its own launch)
    k_kernel_grad_sum<<<dim3(1), dim3(128), 0, st>>>(g->d, g->dpad, g->nparts, g->part.as<const double>(), (const double *)op->k_pts.params, sc, alpha, ch == 0 ? beta : 1.0, g->vals.as<double>());
    HIP_TRY(hipGetLastError());
  }
  g->count += m;
  return SLQ_OK;
}

extern "C" int slq_kernel_grad_get(slq_kernel_grad *g, double *vals, int nvals, int64_t *count) {
  if (!g) return fail(SLQ_EINVAL, "slq_kernel_grad_get: accumulator is NULL");
  if (vals && nvals != g->d + 2) return fail(SLQ_EINVAL, "slq_kernel_grad_get: room for %d values, the accumulator holds d + 2 = %d", nvals, g->d + 2);
  HIP_TRY(hipSetDevice(g->ctx->device));
  if (vals) HIP_TRY(hipMemcpyAsync(vals, g->vals.p, (size_t)(g->d + 2) * 8, hipMemcpyDeviceToHost, g->ctx->stream));
  HIP_TRY(hipStreamSynchronize(g->ctx->stream));
  if (count) *count = g->count;
  return SLQ_OK;
}

extern "C" int slq_kernel_grad_reset(slq_kernel_grad *g) {
  if (!g) return fail(SLQ_EINVAL, "slq_kernel_grad_reset: accumulator is NULL");
  HIP_TRY(hipSetDevice(g->ctx->device));
  HIP_TRY(hipMemsetAsync(g->vals.p, 0, (size_t)(g->d + 2) * 8, g->ctx->stream));
  g->count = 0;
  return SLQ_OK;
}

// kernel_grad_schedule() of slq_kernelgrad.hpp as an array: rows per block, row blocks, columns per chunk, chunks, slabs, then
// slab_begin[0 .. slabs]. No HIP call.
extern "C" int slq_debug_kernel_grad_schedule(int64_t n, int m, int num_cus, int64_t *out, int nout) {
  if (!out || nout < 5 + kKernelMaxSlabs + 1) return fail(SLQ_EINVAL, "slq_debug_kernel_grad_schedule: room for %d values", 5 + kKernelMaxSlabs + 1);
  if (n <= 0 || n >= ((int64_t)1 << 31) - 16 || m <= 0 || num_cus <= 0) return fail(SLQ_EINVAL, "slq_debug_kernel_grad_schedule: 0 < n < 2^31 - 16, m and num_cus positive");
  const KernelGradSchedule S = kernel_grad_schedule(n, m, num_cus);
  kernel_schedule_words({S.rows_per_block, S.nrow_blocks, S.chunk_cols, S.ncol_chunks, S.nslabs}, S.nslabs, S.slab_begin, kKernelMaxSlabs, out);
  return SLQ_OK;
}

// ---- cross-covariance products of the kernel operator (schedule and kernels in slq_kernelcross.hpp) -----------
struct slq_kernel_cross {
  slq_context *ctx = nullptr;
  slq_operator *op = nullptr;  // not owned: read at every product (its z, norms, s and lengthscales as they are then)
  int dtype = SLQ_F64;
  KernelPoints pts;  // the m new points, z*^T (dpad x mpad), |z*|^2 (mpad) and two words k_kernel_rescale writes (never the operator's)
  uint64_t epoch = 0;  // the operator's k_epoch the z* were derived at
  DevBuf scratch;      // slab partials: sized on first use, grown on demand
  DevBuf stage_in, stage_out;  // device copies of the host panels of slq_kernel_cross_matmat (grown on demand)
};

// z*, |z*|^2 from the raw new points with the operator's centre and its lengthscales of now, on the stream (no allocation, no upload)
static int kernel_cross_rescale(slq_kernel_cross *c) {
  HIP_TRY(c->pts.rescale(*c->op->k_scale, c->op->k_s, 0.0, c->dtype, c->ctx->stream));
  c->epoch = c->op->k_epoch;
  return SLQ_OK;
}

static int kernel_cross_create_body(slq_context *ctx, slq_operator *op, int64_t m, const void *points, int64_t ldp, bool on_device, slq_kernel_cross **out) {
  if (!ctx || !op || !points || !out) return fail(SLQ_EINVAL, "slq_kernel_cross_create: ctx/op/points/out is NULL");
  *out = nullptr;
  SLQ_TRY(kernel_base_check(ctx, op, "slq_kernel_cross_create", false, false, false));
  if (m < 1 || m >= ((int64_t)1 << 31) - 16) return fail(SLQ_EINVAL, "slq_kernel_cross_create: m = %lld new points (1 <= m < 2^31 - 16)", (long long)m);
  const int d = op->k_pts.d;
  if (ldp < d) return fail(SLQ_EINVAL, "slq_kernel_cross_create: ldp = %lld is below d = %d", (long long)ldp, d);
  HIP_TRY(hipSetDevice(ctx->device));
  try {
    std::unique_ptr<slq_kernel_cross> c(new slq_kernel_cross());
    c->ctx = ctx, c->op = op, c->dtype = op->dtype;
    KernelBad bad;
    const hipError_t e = c->pts.alloc_and_upload(m, d, points, ldp, on_device, op->dtype, ctx->stream, &bad);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? SLQ_ENOMEM : SLQ_EHIP, "slq_kernel_cross_create: %s", hipGetErrorString(e));
    if (bad.what != KERNEL_OK)
      return fail(SLQ_EINVAL, "slq_kernel_cross_create: new point %lld, coordinate %d is %g (points must be finite)", (long long)bad.row, (int)bad.col, bad.value);
    SLQ_TRY(kernel_cross_rescale(c.get()));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx_retain(ctx);
    *out = c.release();
  } catch (const std::bad_alloc &) {
    return fail(SLQ_ENOMEM, "slq_kernel_cross_create: host allocation failed");
  }
  return SLQ_OK;
}
extern "C" int slq_kernel_cross_create(slq_context *ctx, slq_operator *op, int64_t m, const void *points, int64_t ldp, slq_kernel_cross **out) {
  return kernel_cross_create_body(ctx, op, m, points, ldp, false, out);
}
extern "C" int slq_kernel_cross_create_device(slq_context *ctx, slq_operator *op, int64_t m, const void *d_points, int64_t ldp, slq_kernel_cross **out) {
  return kernel_cross_create_body(ctx, op, m, d_points, ldp, true, out);
}

extern "C" int slq_kernel_cross_destroy(slq_kernel_cross *c) { return handle_destroy(c); }

// The slab scaffold of the cross, feature and adjoint feature products, whose schedules S split the summed side into slabs: more
// than 65535 column chunks are refused (max_cols_msg: the b that still fits), launch(out, ldo, slab_stride) fills the product's own
// args and calls its own *_launch - with one slab straight into Y, else into `scratch` (grown on demand: nslabs partials of
// rows_out x b, packed), which kernel_cross_sum_launch then folds into Y. Everything on the context's stream.
template <typename Launch>
static int slab_product(slq_context *ctx, bool is_f64, const KernelSchedule &S, int64_t rows_out, int b, int max_cols_msg, DevBuf &scratch, void *Y, int64_t ldy,
                        const char *who, Launch launch) {
  if (S.ncol_chunks > 65535) return fail(SLQ_EINVAL, "%s: b = %d columns (at most %d)", who, b, max_cols_msg);
  const int64_t slab_stride = rows_out * (int64_t)b;
  const bool slabs = S.nslabs > 1;
  if (slabs) SLQ_TRY(devbuf_grow(scratch, (size_t)S.nslabs * (size_t)slab_stride * (is_f64 ? 8 : 4), who, "slab scratch"));
  if (!launch(slabs ? scratch.p : Y, slabs ? rows_out : ldy, slab_stride)) return fail(SLQ_EINVAL, "%s: no kernel for %d column tiles", who, S.col_blocks);
  HIP_TRY(hipGetLastError());
  if (slabs) {
    kernel_cross_sum_launch(is_f64, rows_out, b, S.nslabs, scratch.p, slab_stride, Y, ldy, (void *)ctx->stream);
    HIP_TRY(hipGetLastError());
  }
  return SLQ_OK;
}

// Y = C X (trans == 0: X n x b, Y m x b) or C^T X (X m x b, Y n x b) for device arrays, on the stream. The caller has checked the shapes.
static int kernel_cross_product(slq_kernel_cross *c, int trans, const void *X, int64_t ldx, void *Y, int64_t ldy, int b, const char *who) {
  const slq_operator *op = c->op;
  if (c->epoch != op->k_epoch) SLQ_TRY(kernel_cross_rescale(c));  // the hyperparameters have moved: z* follow, before this product
  const bool fwd = trans == 0;
  const int64_t nrows = fwd ? c->pts.n : op->n, nsum = fwd ? op->n : c->pts.n;
  const KernelSchedule S = kernel_cross_schedule(nrows, nsum, b, c->ctx->num_cus);
  KernelCrossArgs a;
  a.nrows = (int)nrows, a.rpad = (int)(fwd ? c->pts.npad : op->k_pts.npad);
  a.nsum = (int)nsum, a.spad = (int)(fwd ? op->k_pts.npad : c->pts.npad);
  a.dq = c->pts.dpad / 4;
  a.rzt = fwd ? c->pts.zt : op->k_pts.zt, a.rnrm = fwd ? c->pts.nrm : op->k_pts.nrm;
  a.szt = fwd ? op->k_pts.zt : c->pts.zt, a.snrm = fwd ? op->k_pts.nrm : c->pts.nrm;
  a.params = op->k_pts.params;
  a.W = X, a.ldw = ldx, a.b = b;
  const bool f64 = c->dtype == SLQ_F64;
  return slab_product(c->ctx, f64, S, nrows, b, 65535 * 16 * kKernelMaxColBlocks, c->scratch, Y, ldy, who, [&](void *out, int64_t ldo, int64_t slab_stride) {
    a.out = out, a.ldo = ldo, a.slab_stride = slab_stride;
    return kernel_cross_launch(f64, op->k_profile, S, a, (void *)c->ctx->stream);
  });
}

extern "C" int slq_kernel_cross_matmat(slq_kernel_cross *c, int trans, const void *X, int64_t ldx, void *Y, int64_t ldy, int b) {
  if (!c) return fail(SLQ_EINVAL, "slq_kernel_cross_matmat: cross object is NULL");
  if (!X || !Y) return fail(SLQ_EINVAL, "slq_kernel_cross_matmat: X/Y is NULL");
  if (trans != 0 && trans != 1) return fail(SLQ_EINVAL, "slq_kernel_cross_matmat: trans = %d (0: Y = C X, 1: Y = C^T X)", trans);
  if (b < 1) return fail(SLQ_EINVAL, "slq_kernel_cross_matmat: b = %d columns (b >= 1)", b);
  const int64_t rin = trans ? c->pts.n : c->op->n, rout = trans ? c->op->n : c->pts.n;
  if (ldx < rin) return fail(SLQ_EINVAL, "slq_kernel_cross_matmat: ldx = %lld is below the %lld rows of X (trans = %d)", (long long)ldx, (long long)rin, trans);
  if (ldy < rout) return fail(SLQ_EINVAL, "slq_kernel_cross_matmat: ldy = %lld is below the %lld rows of Y (trans = %d)", (long long)ldy, (long long)rout, trans);
  return staged_panel_product(c->ctx, esize(c->dtype), c->stage_in, c->stage_out, X, ldx, rin, Y, ldy, rout, b, "slq_kernel_cross_matmat",
                              [&](const void *in, int64_t ld_in, void *out, int64_t ld_out) { return kernel_cross_product(c, trans, in, ld_in, out, ld_out, b, "slq_kernel_cross_matmat"); });
}

extern "C" int slq_kernel_cross_dmat(slq_kernel_cross *c, int trans, slq_dmat *IN, int i0, slq_dmat *OUT, int o0, int b) {
  if (!c) return fail(SLQ_EINVAL, "slq_kernel_cross_dmat: cross object is NULL");
  if (c->dtype != SLQ_F64) return fail(SLQ_EINVAL, "slq_kernel_cross_dmat: the cross object's dtype is fp32: the device matrices are fp64 (use slq_kernel_cross_matmat)");
  if (trans != 0 && trans != 1) return fail(SLQ_EINVAL, "slq_kernel_cross_dmat: trans = %d (0: OUT = C IN, 1: OUT = C^T IN)", trans);
  if (b < 1) return fail(SLQ_EINVAL, "slq_kernel_cross_dmat: b = %d columns (b >= 1)", b);
  const int64_t rin = trans ? c->pts.n : c->op->n, rout = trans ? c->op->n : c->pts.n;
  const double *in;
  double *out;
  SLQ_TRY(dmat_operands(IN, i0, OUT, o0, b, rin, rout, c->ctx, "slq_kernel_cross_dmat", &in, &out));
  HIP_TRY(hipSetDevice(c->ctx->device));
  return kernel_cross_product(c, trans, in, rin, out, rout, b, "slq_kernel_cross_dmat");
}

// z*^T (dpad x mpad, mpad = m rounded up to 16) and |z*|^2 (mpad) in the object's dtype, brought up to the operator's parameters
// of now first - the re-derivation a product would do (tests)
extern "C" int slq_debug_kernel_cross_points(slq_kernel_cross *c, void *zt, void *nrm) {
  if (!c) return fail(SLQ_EINVAL, "slq_debug_kernel_cross_points: cross object is NULL");
  HIP_TRY(hipSetDevice(c->ctx->device));
  if (c->epoch != c->op->k_epoch) SLQ_TRY(kernel_cross_rescale(c));
  HIP_TRY(hipStreamSynchronize(c->ctx->stream));
  HIP_TRY(c->pts.download(zt, nrm, nullptr, c->dtype));
  return SLQ_OK;
}

// kernel_cross_schedule() of slq_kernelcross.hpp as an array: rows per block, row blocks, 16-column tiles per workgroup, column
// chunks, slabs, tiles per slab, then slab_begin[0 .. slabs] (-1 beyond). No HIP call.
extern "C" int slq_debug_kernel_cross_schedule(int64_t nrows, int64_t nsum, int64_t b, int num_cus, int64_t *out, int nout) {
  return kernel_schedule_debug("slq_debug_kernel_cross_schedule", kernel_extents_ok({nrows, nsum, b}, num_cus), "0 < nrows, nsum, b < 2^31 - 16 and num_cus positive", 6,
                               kKernelCrossMaxSlabs, out, nout, [&]() { return kernel_cross_schedule(nrows, nsum, b, num_cus); });
}

// ---- random Fourier features of the kernel operator (schedule and kernel in slq_kernelfeature.hpp) ----------------
struct slq_kernel_feature {
  slq_context *ctx = nullptr;
  slq_operator *op = nullptr;  // not owned: read at every product (its z, its s as they are then)
  int dtype = SLQ_F64;
  int64_t f2 = 0, f2pad = 0;
  int d = 0, dpad = 0;
  DevBuf omt;                  // Omega^T, k-major: dpad x f2pad, zeros in the padding
  DevBuf scratch;              // slab partials: sized on first use, grown on demand
  DevBuf stage_in, stage_out;  // device copies of the host panels of slq_kernel_feature_matmat (grown on demand)
};

template <typename F> static void kernel_feature_transpose(int64_t f2, int64_t f2pad, int d, const F *omega, int64_t ld, F *omt, int64_t *bad_row, int *bad_col) {
  *bad_row = -1, *bad_col = 0;
  for (int64_t j = 0; j < f2; ++j)
    for (int k = 0; k < d; ++k) {
      const F v = omega[j * ld + k];
      if (!std::isfinite(v) && *bad_row < 0) *bad_row = j, *bad_col = k;
      omt[(int64_t)k * f2pad + j] = v;
    }
}

extern "C" int slq_kernel_feature_create(slq_context *ctx, slq_operator *op, int64_t F2, const void *omega, int64_t ld, slq_kernel_feature **out) {
  if (!ctx || !op || !omega || !out) return fail(SLQ_EINVAL, "slq_kernel_feature_create: ctx/op/omega/out is NULL");
  *out = nullptr;
  SLQ_TRY(kernel_base_check(ctx, op, "slq_kernel_feature_create", false, false, true));
  if (F2 < 1 || F2 > kKernelFeatureMaxFreq) return fail(SLQ_EINVAL, "slq_kernel_feature_create: F2 = %lld frequencies (1 <= F2 <= 2^30)", (long long)F2);
  const int d = op->k_pts.d, dpad = op->k_pts.dpad;
  if (ld < d) return fail(SLQ_EINVAL, "slq_kernel_feature_create: ld = %lld is below d = %d", (long long)ld, d);
  HIP_TRY(hipSetDevice(ctx->device));
  try {
    std::unique_ptr<slq_kernel_feature> f(new slq_kernel_feature());
    f->ctx = ctx, f->op = op, f->dtype = op->dtype, f->f2 = F2, f->f2pad = kernel_npad(F2), f->d = d, f->dpad = dpad;
    const size_t es = esize(op->dtype), words = (size_t)dpad * (size_t)f->f2pad;
    std::vector<char> host(words * es, 0);
    int64_t bad_row;
    int bad_col;
    if (op->dtype == SLQ_F64) kernel_feature_transpose<double>(F2, f->f2pad, d, (const double *)omega, ld, (double *)host.data(), &bad_row, &bad_col);
    else kernel_feature_transpose<float>(F2, f->f2pad, d, (const float *)omega, ld, (float *)host.data(), &bad_row, &bad_col);
    if (bad_row >= 0)
      return fail(SLQ_EINVAL, "slq_kernel_feature_create: frequency %lld, coordinate %d is not finite (frequencies must be finite)", (long long)bad_row, bad_col);
    const hipError_t e = f->omt.alloc(words * es);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? SLQ_ENOMEM : SLQ_EHIP, "slq_kernel_feature_create: %s", hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(f->omt.p, host.data(), words * es, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // (the host copy goes with this frame)
    ctx_retain(ctx);
    *out = f.release();
  } catch (const std::bad_alloc &) {
    return fail(SLQ_ENOMEM, "slq_kernel_feature_create: host allocation failed");
  }
  return SLQ_OK;
}

extern "C" int slq_kernel_feature_destroy(slq_kernel_feature *f) { return handle_destroy(f); }

// the row points of a product: the operator's own (cross NULL) or the new points of a cross object of the same operator
static int kernel_feature_rows(const slq_kernel_feature *f, const slq_kernel_cross *cross, const char *who) {
  if (cross && cross->op != f->op) return fail(SLQ_EINVAL, "%s: the cross object belongs to another operator than the feature map", who);
  return SLQ_OK;
}

// Y = Phi W for device arrays (W 2 F2 x b, Y rows x b), on the stream. The caller has checked the shapes.
static int kernel_feature_product_run(slq_kernel_feature *f, slq_kernel_cross *cross, const void *W, int64_t ldw, void *Y, int64_t ldy, int b, const char *who) {
  const slq_operator *op = f->op;
  if (cross && cross->epoch != op->k_epoch) SLQ_TRY(kernel_cross_rescale(cross));  // the hyperparameters have moved: z* follow, before this product
  const KernelPoints &pts = cross ? cross->pts : op->k_pts;
  const bool f64 = f->dtype == SLQ_F64;
  const int64_t nrows = pts.n;
  const KernelSchedule S = kernel_feature_schedule(nrows, f->f2, b, f->ctx->num_cus, f64);
  KernelFeatureArgs a;
  a.nrows = (int)nrows, a.rpad = (int)pts.npad;
  a.nfreq = (int)f->f2, a.fpad = (int)f->f2pad;
  a.dq = f->dpad / 4;
  a.rzt = pts.zt, a.rnrm = pts.nrm;
  a.omt = f->omt.p;
  a.params = op->k_pts.params;
  a.W = W, a.ldw = ldw, a.b = b;
  return slab_product(f->ctx, f64, S, nrows, b, 65535 * kernel_feature_chunk_cols(f64), f->scratch, Y, ldy, who, [&](void *out, int64_t ldo, int64_t slab_stride) {
    a.out = out, a.ldo = ldo, a.slab_stride = slab_stride;
    return kernel_feature_launch(f64, S, a, (void *)f->ctx->stream);
  });
}

extern "C" int slq_kernel_feature_matmat(slq_kernel_feature *f, slq_kernel_cross *cross, const void *W, int64_t ldw, void *Y, int64_t ldy, int b) {
  if (!f) return fail(SLQ_EINVAL, "slq_kernel_feature_matmat: feature map is NULL");
  if (!W || !Y) return fail(SLQ_EINVAL, "slq_kernel_feature_matmat: W/Y is NULL");
  SLQ_TRY(kernel_feature_rows(f, cross, "slq_kernel_feature_matmat"));
  if (b < 1) return fail(SLQ_EINVAL, "slq_kernel_feature_matmat: b = %d columns (b >= 1)", b);
  const int64_t rin = 2 * f->f2, rout = cross ? cross->pts.n : f->op->n;
  if (ldw < rin) return fail(SLQ_EINVAL, "slq_kernel_feature_matmat: ldw = %lld is below the %lld rows of W (2 F2)", (long long)ldw, (long long)rin);
  if (ldy < rout) return fail(SLQ_EINVAL, "slq_kernel_feature_matmat: ldy = %lld is below the %lld rows of Y", (long long)ldy, (long long)rout);
  return staged_panel_product(f->ctx, esize(f->dtype), f->stage_in, f->stage_out, W, ldw, rin, Y, ldy, rout, b, "slq_kernel_feature_matmat",
                              [&](const void *in, int64_t ld_in, void *out, int64_t ld_out) { return kernel_feature_product_run(f, cross, in, ld_in, out, ld_out, b, "slq_kernel_feature_matmat"); });
}

extern "C" int slq_kernel_feature_dmat(slq_kernel_feature *f, slq_kernel_cross *cross, slq_dmat *IN, int i0, slq_dmat *OUT, int o0, int b) {
  if (!f) return fail(SLQ_EINVAL, "slq_kernel_feature_dmat: feature map is NULL");
  if (f->dtype != SLQ_F64) return fail(SLQ_EINVAL, "slq_kernel_feature_dmat: the feature map's dtype is fp32: the device matrices are fp64 (use slq_kernel_feature_matmat)");
  SLQ_TRY(kernel_feature_rows(f, cross, "slq_kernel_feature_dmat"));
  if (b < 1) return fail(SLQ_EINVAL, "slq_kernel_feature_dmat: b = %d columns (b >= 1)", b);
  const int64_t rin = 2 * f->f2, rout = cross ? cross->pts.n : f->op->n;
  const double *in;
  double *out;
  SLQ_TRY(dmat_operands(IN, i0, OUT, o0, b, rin, rout, f->ctx, "slq_kernel_feature_dmat", &in, &out));
  HIP_TRY(hipSetDevice(f->ctx->device));
  return kernel_feature_product_run(f, cross, in, rin, out, rout, b, "slq_kernel_feature_dmat");
}

// Z = Phi^T U for device arrays (U rows x b, Z 2 F2 x b), on the stream. The caller has checked the shapes.
static int kernel_feature_adjoint_run(slq_kernel_feature *f, slq_kernel_cross *cross, const void *U, int64_t ldu, void *Z, int64_t ldz, int b, const char *who) {
  const slq_operator *op = f->op;
  if (cross && cross->epoch != op->k_epoch) SLQ_TRY(kernel_cross_rescale(cross));  // the hyperparameters have moved: z* follow, before this product
  const KernelPoints &pts = cross ? cross->pts : op->k_pts;
  const bool f64 = f->dtype == SLQ_F64;
  const int64_t nrows = pts.n, rout = 2 * f->f2;
  const KernelSchedule S = kernel_feature_adjoint_schedule(f->f2, nrows, b, f->ctx->num_cus, f64);
  KernelFeatureAdjArgs a;
  a.nfreq = (int)f->f2, a.fpad = (int)f->f2pad;
  a.nrows = (int)nrows, a.rpad = (int)pts.npad;
  a.dq = f->dpad / 4;
  a.omt = f->omt.p, a.rzt = pts.zt;
  a.params = op->k_pts.params;
  a.U = U, a.ldu = ldu, a.b = b;
  return slab_product(f->ctx, f64, S, rout, b, 65535 * kernel_feature_adjoint_chunk_cols(f64), f->scratch, Z, ldz, who, [&](void *out, int64_t ldo, int64_t slab_stride) {
    a.out = out, a.ldo = ldo, a.slab_stride = slab_stride;
    return kernel_feature_adjoint_launch(f64, S, a, (void *)f->ctx->stream);
  });
}

extern "C" int slq_kernel_feature_rmatmat(slq_kernel_feature *f, slq_kernel_cross *cross, const void *U, int64_t ldu, void *Z, int64_t ldz, int b) {
  if (!f) return fail(SLQ_EINVAL, "slq_kernel_feature_rmatmat: feature map is NULL");
  if (!U || !Z) return fail(SLQ_EINVAL, "slq_kernel_feature_rmatmat: U/Z is NULL");
  SLQ_TRY(kernel_feature_rows(f, cross, "slq_kernel_feature_rmatmat"));
  if (b < 1) return fail(SLQ_EINVAL, "slq_kernel_feature_rmatmat: b = %d columns (b >= 1)", b);
  const int64_t rin = cross ? cross->pts.n : f->op->n, rout = 2 * f->f2;
  if (ldu < rin) return fail(SLQ_EINVAL, "slq_kernel_feature_rmatmat: ldu = %lld is below the %lld rows of U", (long long)ldu, (long long)rin);
  if (ldz < rout) return fail(SLQ_EINVAL, "slq_kernel_feature_rmatmat: ldz = %lld is below the %lld rows of Z (2 F2)", (long long)ldz, (long long)rout);
  return staged_panel_product(f->ctx, esize(f->dtype), f->stage_in, f->stage_out, U, ldu, rin, Z, ldz, rout, b, "slq_kernel_feature_rmatmat",
                              [&](const void *in, int64_t ld_in, void *out, int64_t ld_out) { return kernel_feature_adjoint_run(f, cross, in, ld_in, out, ld_out, b, "slq_kernel_feature_rmatmat"); });
}

extern "C" int slq_kernel_feature_rdmat(slq_kernel_feature *f, slq_kernel_cross *cross, slq_dmat *IN, int i0, slq_dmat *OUT, int o0, int b) {
  if (!f) return fail(SLQ_EINVAL, "slq_kernel_feature_rdmat: feature map is NULL");
  if (f->dtype != SLQ_F64) return fail(SLQ_EINVAL, "slq_kernel_feature_rdmat: the feature map's dtype is fp32: the device matrices are fp64 (use slq_kernel_feature_rmatmat)");
  SLQ_TRY(kernel_feature_rows(f, cross, "slq_kernel_feature_rdmat"));
  if (b < 1) return fail(SLQ_EINVAL, "slq_kernel_feature_rdmat: b = %d columns (b >= 1)", b);
  const int64_t rin = cross ? cross->pts.n : f->op->n, rout = 2 * f->f2;
  const double *in;
  double *out;
  SLQ_TRY(dmat_operands(IN, i0, OUT, o0, b, rin, rout, f->ctx, "slq_kernel_feature_rdmat", &in, &out));
  HIP_TRY(hipSetDevice(f->ctx->device));
  return kernel_feature_adjoint_run(f, cross, in, rin, out, rout, b, "slq_kernel_feature_rdmat");
}

// kernel_feature_adjoint_schedule() of slq_kernelfeatureadj.hpp as an array, in the order of slq_debug_kernel_feature_schedule (the
// row blocks are those of the frequencies, the slabs those of the row points). No HIP call.
extern "C" int slq_debug_kernel_feature_adjoint_schedule(int64_t F2, int64_t nrows, int64_t b, int num_cus, int is_f64, int64_t *out, int nout) {
  return kernel_schedule_debug("slq_debug_kernel_feature_adjoint_schedule", kernel_extents_ok({nrows, F2, b}, num_cus) && F2 <= kKernelFeatureMaxFreq,
                               "0 < nrows, b < 2^31 - 16, 0 < F2 <= 2^30 and num_cus positive", 6, kKernelCrossMaxSlabs, out, nout,
                               [&]() { return kernel_feature_adjoint_schedule(F2, nrows, b, num_cus, is_f64 != 0); });
}

// Omega^T as the device holds it: dpad x F2pad in the object's dtype (tests: the padding must be zero)
extern "C" int slq_debug_kernel_feature_frequencies(slq_kernel_feature *f, void *omega_t) {
  if (!f || !omega_t) return fail(SLQ_EINVAL, "slq_debug_kernel_feature_frequencies: feature map / omega_t is NULL");
  HIP_TRY(hipSetDevice(f->ctx->device));
  HIP_TRY(hipStreamSynchronize(f->ctx->stream));
  HIP_TRY(hipMemcpy(omega_t, f->omt.p, (size_t)f->dpad * (size_t)f->f2pad * esize(f->dtype), hipMemcpyDeviceToHost));
  return SLQ_OK;
}

// kernel_feature_schedule() of slq_kernelfeature.hpp as an array, in the order of slq_debug_kernel_cross_schedule. No HIP call.
extern "C" int slq_debug_kernel_feature_schedule(int64_t nrows, int64_t F2, int64_t b, int num_cus, int is_f64, int64_t *out, int nout) {
  return kernel_schedule_debug("slq_debug_kernel_feature_schedule", kernel_extents_ok({nrows, F2, b}, num_cus) && F2 <= kKernelFeatureMaxFreq,
                               "0 < nrows, b < 2^31 - 16, 0 < F2 <= 2^30 and num_cus positive", 6, kKernelCrossMaxSlabs, out, nout,
                               [&]() { return kernel_feature_schedule(nrows, F2, b, num_cus, is_f64 != 0); });
}

// ---- pivoted-Cholesky preconditioner of a kernel operator (kernels and host analysis in slq_kernelprecond.hpp) ----
static int precond_handle(const slq_operator *op, const char *who) {
  if (!op) return fail(SLQ_EINVAL, "%s: the operator is NULL", who);
  if (op->kind != OP_KERNEL_PRECOND || !op->pre)
    return fail(SLQ_EINVAL, "%s: the operator is of kind '%s', not a preconditioned kernel operator (slq_kernel_precond_create)", who, op_kind_name(op->kind));
  return SLQ_OK;
}

// The factor of the base's K0 as its hyperparameters are now, in place: rank_max steps back to back on the stream, the Gram
// matrix L^T L by the apply's own kernel with L as the panel, then - after the one synchronisation - Jacobi, G and logdet P
// on the host, and G uploaded to its fixed address.
static int precond_factorise(slq_operator *op) {
  KernelPrecond &pc = *op->pre;
  const slq_operator *base = pc.base;
  if (!(base->k_noise > 0.0)) return fail(SLQ_EINVAL, "kernel preconditioner: the base operator's noise sigma2 is 0: P^{-1/2} needs sigma2 > 0");
  hipStream_t st = op->ctx->stream;
  const int n = (int)op->n, r = pc.rank_max, rpad = pc.rpad, cus = op->ctx->num_cus;
  HIP_TRY(hipStreamSynchronize(st));  // (what ran before is not this factorisation's time)
  const auto t0 = std::chrono::steady_clock::now();
  HIP_TRY(hipMemsetAsync(pc.L.p, 0, (size_t)n * rpad * 8, st));
  const double thresh = std::max(pc.tol, 64.0 * std::numeric_limits<double>::epsilon());
  if (!precond_factor_launch(base->k_profile, n, (int)base->k_pts.npad, base->k_pts.d, (const double *)base->k_pts.zt, (const double *)base->k_pts.nrm,
                             (const double *)base->k_pts.params, pc.L.as<double>(), rpad, r, thresh, pc.dres.as<double>(), pc.pivots, pc.rank_d, pc.dpiv, pc.pv, pc.pi, st))
    return fail(SLQ_EINVAL, "kernel preconditioner: no factor kernel for profile %d", base->k_profile);
  HIP_TRY(hipGetLastError());
  SLQ_TRY(devbuf_grow(pc.scratch, precond_scratch_words(n, rpad, rpad, cus) * 8, "kernel preconditioner"));
  const PrecondSlabs S = precond_apply_slabs(n, rpad, cus);
  const size_t bpad = (size_t)precond_bpad(rpad);
  double *gram_d = pc.scratch.as<double>() + (size_t)S.nslabs * bpad * rpad;
  if (!precond_lt_launch(n, pc.L.as<const double>(), rpad, (const double *)nullptr, pc.L.as<const double>(), rpad, PrecondPanelLayout{n, rpad}, pc.scratch.as<double>(), gram_d,
                         cus, st))
    return fail(SLQ_EINVAL, "kernel preconditioner: no Gram kernel for rank %d", rpad);
  HIP_TRY(hipGetLastError());
  std::vector<double> gram((size_t)rpad * rpad), dres((size_t)n), A((size_t)r * r), V((size_t)r * r), t((size_t)r), G((size_t)rpad * rpad), H((size_t)rpad * rpad);
  HIP_TRY(hipMemcpyAsync(gram.data(), gram_d, gram.size() * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(dres.data(), pc.dres.p, dres.size() * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&pc.rank, pc.rank_d, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const auto t1 = std::chrono::steady_clock::now();
  for (int i = 0; i < r; ++i)
    for (int j = i; j < r; ++j) A[(size_t)i * r + j] = A[(size_t)j * r + i] = gram[(size_t)i * rpad + j];  // (gram[g][m]: column g of the product, symmetric)
  if (precond_jacobi(r, A.data(), V.data(), t.data()) >= kPrecondJacobiSweeps) return fail(SLQ_ENOTCONV, "kernel preconditioner: Jacobi did not converge on the %d x %d Gram matrix", r, r);
  const PrecondSpectrum sp = precond_finish(n, r, rpad, V.data(), t.data(), base->k_noise, G.data(), H.data());
  HIP_TRY(hipMemcpyAsync(pc.G.p, G.data(), G.size() * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(pc.H.p, H.data(), H.size() * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  const auto t2 = std::chrono::steady_clock::now();
  pc.device_ms = std::chrono::duration<double, std::milli>(t1 - t0).count(), pc.host_ms = std::chrono::duration<double, std::milli>(t2 - t1).count();
  pc.logdet_p = sp.logdet_p, pc.t_max = sp.t_max;
  pc.residual_trace = 0.0;
  for (double v : dres) pc.residual_trace += v;
  pc.eig = t;
  pc.epoch = base->k_epoch;
  return SLQ_OK;
}

static int kernel_precond_create_body(slq_context *ctx, slq_operator *base, int rank_max, double tol, slq_operator **out) {
  if (!ctx || !base || !out) return fail(SLQ_EINVAL, "slq_kernel_precond_create: ctx/kernel_op/out is NULL");
  *out = nullptr;
  SLQ_TRY(kernel_base_check(ctx, base, "slq_kernel_precond_create", true, true, false));
  if (!(base->k_noise > 0.0)) return fail(SLQ_EINVAL, "slq_kernel_precond_create: the base operator's noise sigma2 is 0: P^{-1/2} needs sigma2 > 0");
  if (rank_max < 1 || rank_max > kPrecondMaxRank) return fail(SLQ_EINVAL, "slq_kernel_precond_create: rank_max = %d (1 <= rank_max <= %d)", rank_max, kPrecondMaxRank);
  if (!(tol >= 0.0) || !std::isfinite(tol)) return fail(SLQ_EINVAL, "slq_kernel_precond_create: tol = %g (finite, >= 0)", tol);
  rank_max = (int)std::min<int64_t>(rank_max, base->n);
  slq_operator *op = nullptr;
  SLQ_TRY(operator_new(ctx, OP_KERNEL_PRECOND, SLQ_F64, base->n, base->n * rank_max, out, &op));
  OpGuard guard{op};
  op->pre.reset(new KernelPrecond());
  KernelPrecond &pc = *op->pre;
  pc.base = base, pc.rank_max = rank_max, pc.rpad = precond_rpad(rank_max), pc.tol = tol;
  const size_t n = (size_t)base->n, nparts = (size_t)precond_factor_parts(base->n);
  const size_t head_ints = ((size_t)rank_max + 1 + 1) / 2 * 2;  // pivots | rank, padded to whole doubles
  hipError_t e = pc.L.alloc(n * pc.rpad * 8);
  if (e == hipSuccess) e = pc.G.alloc((size_t)pc.rpad * pc.rpad * 8);
  if (e == hipSuccess) e = pc.H.alloc((size_t)pc.rpad * pc.rpad * 8);
  if (e == hipSuccess) e = pc.dres.alloc(n * 8);
  if (e == hipSuccess) e = pc.words.alloc(head_ints * 4 + ((size_t)rank_max + 2 * nparts) * 8 + 2 * nparts * 4);
  if (e == hipSuccess) e = hipMemsetAsync(pc.G.p, 0, (size_t)pc.rpad * pc.rpad * 8, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(pc.H.p, 0, (size_t)pc.rpad * pc.rpad * 8, ctx->stream);
  if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? SLQ_ENOMEM : SLQ_EHIP, "slq_kernel_precond_create: %s", hipGetErrorString(e));
  pc.pivots = pc.words.as<int>(), pc.rank_d = pc.pivots + rank_max;
  pc.dpiv = (double *)(pc.pivots + head_ints), pc.pv = pc.dpiv + rank_max;
  pc.pi = (int *)(pc.pv + 2 * nparts);
  SLQ_TRY(precond_factorise(op));
  *out = guard.release();
  return SLQ_OK;
}
extern "C" int slq_kernel_precond_create(slq_context *ctx, slq_operator *kernel_op, int rank_max, double tol, slq_operator **out) {
  return create_guarded(out, [&]() { return kernel_precond_create_body(ctx, kernel_op, rank_max, tol, out); });
}

extern "C" int slq_kernel_precond_refresh(slq_operator *op) {
  SLQ_TRY(precond_handle(op, "slq_kernel_precond_refresh"));
  SLQ_TRY(kernel_refuse_scaled(op->pre->base, "slq_kernel_precond_refresh"));
  HIP_TRY(hipSetDevice(op->ctx->device));
  return create_guarded(nullptr, [&]() { return precond_factorise(op); });
}

extern "C" int slq_kernel_precond_info(const slq_operator *op, int *rank_max, int *rank, double *logdet_p, double *residual_trace, double *t_max) {
  SLQ_TRY(precond_handle(op, "slq_kernel_precond_info"));
  const KernelPrecond &pc = *op->pre;
  if (rank_max) *rank_max = pc.rank_max;
  if (rank) *rank = pc.rank;
  if (logdet_p) *logdet_p = pc.logdet_p;
  if (residual_trace) *residual_trace = pc.residual_trace;
  if (t_max) *t_max = pc.t_max;
  return SLQ_OK;
}

extern "C" int slq_kernel_precond_get(slq_operator *op, int32_t *pivots, double *L, int64_t ldl, double *G, double *eig) {
  SLQ_TRY(precond_handle(op, "slq_kernel_precond_get"));
  const KernelPrecond &pc = *op->pre;
  if (L && ldl < op->n) return fail(SLQ_EINVAL, "slq_kernel_precond_get: ldl = %lld is below n = %lld", (long long)ldl, (long long)op->n);
  HIP_TRY(hipSetDevice(op->ctx->device));
  HIP_TRY(hipStreamSynchronize(op->ctx->stream));
  return create_guarded(nullptr, [&]() {
    const size_t n = (size_t)op->n, r = (size_t)pc.rank_max, rpad = (size_t)pc.rpad;
    if (pivots) HIP_TRY(hipMemcpy(pivots, pc.pivots, r * 4, hipMemcpyDeviceToHost));
    if (L) {
      std::vector<double> rows(n * rpad);
      HIP_TRY(hipMemcpy(rows.data(), pc.L.p, rows.size() * 8, hipMemcpyDeviceToHost));
      for (size_t k = 0; k < r; ++k)
        for (size_t i = 0; i < n; ++i) L[k * (size_t)ldl + i] = rows[i * rpad + k];
    }
    if (G) {
      std::vector<double> g(rpad * rpad);
      HIP_TRY(hipMemcpy(g.data(), pc.G.p, g.size() * 8, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < r; ++i) std::copy(g.begin() + i * rpad, g.begin() + i * rpad + r, G + i * r);
    }
    if (eig) std::copy(pc.eig.begin(), pc.eig.end(), eig);
    return (int)SLQ_OK;
  });
}

// Y = M X on device columns n apart, on the stream (the caller has checked the shapes)
static int precond_apply_device(slq_operator *op, const double *X, double *Y, int b, const char *who) {
  SLQ_TRY(precond_check_fresh(op, who));
  KernelPrecond &pc = *op->pre;
  const int cus = op->ctx->num_cus;
  SLQ_TRY(devbuf_grow(pc.scratch, precond_scratch_words(op->n, b, pc.rpad, cus) * 8, who));
  if (!precond_apply_launch((int)op->n, pc.L.as<const double>(), pc.rpad, pc.G.as<const double>(), (const double *)pc.base->k_pts.params, X, Y, b,
                            PrecondColumnLayout{op->n}, pc.scratch.as<double>(), cus, op->ctx->stream))
    return fail(SLQ_EINVAL, "%s: no apply kernel for rank %d", who, pc.rpad);
  HIP_TRY(hipGetLastError());
  return SLQ_OK;
}

extern "C" int slq_kernel_precond_apply(slq_operator *op, const void *X, int64_t ldx, void *Y, int64_t ldy, int b) {
  SLQ_TRY(precond_handle(op, "slq_kernel_precond_apply"));
  if (!X || !Y) return fail(SLQ_EINVAL, "slq_kernel_precond_apply: X/Y is NULL");
  if (b < 1) return fail(SLQ_EINVAL, "slq_kernel_precond_apply: b = %d columns (b >= 1)", b);
  if (ldx < op->n || ldy < op->n) return fail(SLQ_EINVAL, "slq_kernel_precond_apply: ldx = %lld, ldy = %lld must reach n = %lld", (long long)ldx, (long long)ldy, (long long)op->n);
  return staged_panel_product(op->ctx, 8, op->pre->stage_in, op->pre->stage_out, X, ldx, op->n, Y, ldy, op->n, b, "slq_kernel_precond_apply",
                              [&](const void *in, int64_t, void *out, int64_t) { return precond_apply_device(op, (const double *)in, (double *)out, b, "slq_kernel_precond_apply"); });
}

extern "C" int slq_kernel_precond_apply_dmat(slq_operator *op, slq_dmat *IN, int i0, slq_dmat *OUT, int o0, int b) {
  SLQ_TRY(precond_handle(op, "slq_kernel_precond_apply_dmat"));
  if (b < 1) return fail(SLQ_EINVAL, "slq_kernel_precond_apply_dmat: b = %d columns (b >= 1)", b);
  const double *in;
  double *out;
  SLQ_TRY(dmat_operands(IN, i0, OUT, o0, b, op->n, op->n, op->ctx, "slq_kernel_precond_apply_dmat", &in, &out));
  HIP_TRY(hipSetDevice(op->ctx->device));
  return precond_apply_device(op, in, out, b, "slq_kernel_precond_apply_dmat");
}

// ---- the factor's columns as operands of the gradient kernel, and the exact part tr(P^-1 dA/dtheta) ----
// columns [c0, c0 + nc) of L (Q null) or L H into a device array of n x nc, column-major; the caller has checked everything
static int precond_columns_device(slq_operator *op, int which, int c0, int nc, double *OUT, const char *who) {
  const KernelPrecond &pc = *op->pre;
  if (!precond_columns_launch((int)op->n, pc.L.as<const double>(), pc.rpad, which ? pc.H.as<const double>() : (const double *)nullptr, c0, nc, OUT, op->ctx->stream))
    return fail(SLQ_EINVAL, "%s: no column kernel for rank %d", who, pc.rpad);
  HIP_TRY(hipGetLastError());
  return SLQ_OK;
}

extern "C" int slq_kernel_precond_columns(slq_operator *op, int which, int c0, int nc, slq_dmat *OUT, int o0) {
  SLQ_TRY(precond_handle(op, "slq_kernel_precond_columns"));
  SLQ_TRY(precond_check_fresh(op, "slq_kernel_precond_columns"));
  const KernelPrecond &pc = *op->pre;
  if (which != 0 && which != 1) return fail(SLQ_EINVAL, "slq_kernel_precond_columns: which = %d (0: L, 1: L H)", which);
  if (c0 < 0 || nc < 1 || nc > kPrecondChunkCols || c0 + nc > pc.rpad)
    return fail(SLQ_EINVAL, "slq_kernel_precond_columns: the column range [%d, %d) is outside [0, rpad = %d) or holds more than %d columns", c0, c0 + nc, pc.rpad, kPrecondChunkCols);
  SLQ_TRY(dmat_range(OUT, o0, nc, "slq_kernel_precond_columns(OUT)"));
  if (OUT->n != op->n) return fail(SLQ_EINVAL, "slq_kernel_precond_columns: row mismatch: the operator has %lld rows, OUT %lld", (long long)op->n, (long long)OUT->n);
  if (OUT->ctx != op->ctx) return fail(SLQ_EINVAL, "slq_kernel_precond_columns: OUT belongs to another context");
  HIP_TRY(hipSetDevice(op->ctx->device));
  return precond_columns_device(op, which, c0, nc, OUT->d + (size_t)o0 * OUT->n, "slq_kernel_precond_columns");
}

// vals = beta vals + alpha sigma^-2 [tr D - sum_c (L H)_c^T D L_c] over the columns of the rank reached, 64 at a time: per chunk two
// column launches and one accumulator update (alpha_u = -alpha / sigma2; beta for the first chunk, 1 after it), then ONE one-thread
// kernel adds alpha n / sigma2 to the outputscale's and the noise's value - everything on the stream, nothing is read back. The
// accumulator's column count is left as it was: no probe was folded in.
// The column loop of the two exact-part entries below, after their own checks of the accumulator: a fresh factor, finite weights,
// then the columns of the rank reached, kPrecondChunkCols at a time, as two views Z = (L H)_c, W = L_c of pc.cols (grown on demand):
// two column launches and update(Z, W, nc, -alpha / sigma2, beta for the first chunk and 1 after it) - the accumulator's own update.
template <typename Update> static int precond_trace_columns(slq_operator *op, const char *who, double alpha, double beta, Update update) {
  KernelPrecond &pc = *op->pre;
  SLQ_TRY(precond_check_fresh(op, who));
  if (!std::isfinite(alpha) || !std::isfinite(beta)) return fail(SLQ_EINVAL, "%s: alpha = %g, beta = %g must be finite", who, alpha, beta);
  HIP_TRY(hipSetDevice(op->ctx->device));
  const size_t n = (size_t)op->n;
  SLQ_TRY(devbuf_grow(pc.cols, 2 * n * kPrecondChunkCols * 8, who));
  slq_dmat Z{op->ctx, op->n, kPrecondChunkCols, pc.cols.as<double>()}, W{op->ctx, op->n, kPrecondChunkCols, pc.cols.as<double>() + n * kPrecondChunkCols};
  const double sigma2 = pc.base->k_noise;
  for (int c0 = 0; c0 < pc.rank; c0 += kPrecondChunkCols) {  // (the rank reached is at least 1: the first pivot's residual is s itself)
    const int nc = std::min(kPrecondChunkCols, pc.rank - c0);
    SLQ_TRY(precond_columns_device(op, 1, c0, nc, Z.d, who));
    SLQ_TRY(precond_columns_device(op, 0, c0, nc, W.d, who));
    SLQ_TRY(update(&Z, &W, nc, -alpha / sigma2, c0 == 0 ? beta : 1.0));
  }
  return SLQ_OK;
}

extern "C" int slq_kernel_precond_trace_grad(slq_operator *op, slq_kernel_grad *g, double alpha, double beta) {
  SLQ_TRY(precond_handle(op, "slq_kernel_precond_trace_grad"));
  if (!g) return fail(SLQ_EINVAL, "slq_kernel_precond_trace_grad: the accumulator is NULL");
  KernelPrecond &pc = *op->pre;
  if (g->op != pc.base) return fail(SLQ_EINVAL, "slq_kernel_precond_trace_grad: the accumulator belongs to another operator: create it on the base of this preconditioned operator");
  const int64_t count = g->count;
  SLQ_TRY(precond_trace_columns(op, "slq_kernel_precond_trace_grad", alpha, beta,
                                [&](slq_dmat *Z, slq_dmat *W, int nc, double a, double b) { return slq_kernel_grad_update(g, Z, 0, W, 0, nc, a, b); }));
  g->count = count;
  hipStream_t st = op->ctx->stream;
  k_precond_trace_add<<<dim3(1), dim3(64), 0, st>>>(g->d, (double)op->n, (const double *)pc.base->k_pts.params, alpha, g->vals.as<double>());
  HIP_TRY(hipGetLastError());
  return SLQ_OK;
}

// ---- gradients with respect to the points (schedule and kernels in slq_kernelpointgrad.hpp) ------------------------
struct slq_kernel_pointgrad {
  slq_context *ctx;
  slq_operator *op;         // not owned: read at every update (its z, norms and scalars as they are then)
  slq_kernel_cross *cross;  // not owned; null: the training form. Else the cross form: the rows are its new points
  int64_t nrows, nsum, count;
  int d, dpad;
  DevBuf vals;  // nrows x d doubles, row-major like the points
  DevBuf part;  // nslabs x nrows x dpad doubles: one partial per slab of a pass
  size_t vals_bytes() const { return (size_t)nrows * (size_t)d * 8; }
};

static int kernel_pointgrad_create_body(slq_context *ctx, slq_operator *op, slq_kernel_cross *cross, const char *who, slq_kernel_pointgrad **out) {
  *out = nullptr;
  SLQ_TRY(kernel_base_check(ctx, op, who, true, !cross, true));  // (the cross form is defined on K0's points and profile, as a cross product is: a scale does not stop it)
  HIP_TRY(hipSetDevice(ctx->device));
  const int64_t nrows = cross ? cross->pts.n : op->n;
  const KernelPointGradSchedule S = kernel_pointgrad_schedule(nrows, op->n, ctx->num_cus);
  std::unique_ptr<slq_kernel_pointgrad> g(new (std::nothrow) slq_kernel_pointgrad{ctx, op, cross, nrows, op->n, 0, op->k_pts.d, op->k_pts.dpad, {}, {}});
  if (!g) return fail(SLQ_ENOMEM, "host allocation failed");
  hipError_t e = g->vals.alloc(g->vals_bytes());
  if (e == hipSuccess) e = g->part.alloc((size_t)S.nslabs * (size_t)nrows * (size_t)g->dpad * 8);
  if (e == hipSuccess) e = hipMemsetAsync(g->vals.p, 0, g->vals_bytes(), ctx->stream);
  if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? SLQ_ENOMEM : SLQ_EHIP, "%s: %s", who, hipGetErrorString(e));
  ctx_retain(ctx);
  *out = g.release();
  return SLQ_OK;
}
extern "C" int slq_kernel_pointgrad_create(slq_context *ctx, slq_operator *op, slq_kernel_pointgrad **out) {
  if (!ctx || !op || !out) return fail(SLQ_EINVAL, "slq_kernel_pointgrad_create: ctx/op/out is NULL");
  return kernel_pointgrad_create_body(ctx, op, nullptr, "slq_kernel_pointgrad_create", out);
}
extern "C" int slq_kernel_pointgrad_create_cross(slq_context *ctx, slq_kernel_cross *cross, slq_kernel_pointgrad **out) {
  if (!ctx || !cross || !out) return fail(SLQ_EINVAL, "slq_kernel_pointgrad_create_cross: ctx/cross/out is NULL");
  return kernel_pointgrad_create_body(ctx, cross->op, cross, "slq_kernel_pointgrad_create_cross", out);
}

extern "C" int slq_kernel_pointgrad_destroy(slq_kernel_pointgrad *g) { return handle_destroy(g); }

// one pass of k_kernel_pointgrad and its fold: vals = beta vals + alpha R(U, W) over mc <= 64 columns
static int kernel_pointgrad_pass(slq_kernel_pointgrad *g, const KernelPointGradSchedule &S, const KernelPointGradScale &sc, const double *U, const double *W,
                                 int mc, double alpha, double beta) {
  const slq_operator *op = g->op;
  const KernelPoints &rows = g->cross ? g->cross->pts : op->k_pts;
  const KernelPointGradArgs a{(int)g->nrows, (int)rows.npad, (int)g->nsum, (int)op->k_pts.npad, g->dpad / 4, g->cross ? 0 : 1,
                              (const double *)rows.zt, (const double *)rows.nrm, (const double *)op->k_pts.zt, (const double *)op->k_pts.nrm,
                              U, W, mc, g->part.as<double>()};
  if (!kernel_pointgrad_launch(op->k_profile, S, a, (void *)g->ctx->stream)) return fail(SLQ_EINVAL, "slq_kernel_pointgrad_update: no kernel for profile %d", op->k_profile);
  HIP_TRY(hipGetLastError());
  // (the passes run one after the other on the stream: each fold reads the partials of its own pass)
  kernel_pointgrad_sum_launch(g->nrows, g->d, g->dpad, S.nslabs, g->part.as<const double>(), (const double *)op->k_pts.params, sc, alpha, beta, g->vals.as<double>(),
                              (void *)g->ctx->stream);
  HIP_TRY(hipGetLastError());
  return SLQ_OK;
}

extern "C" int slq_kernel_pointgrad_update(slq_kernel_pointgrad *g, slq_dmat *Z, int z0, slq_dmat *W, int w0, int m, double alpha, double beta) {
  if (!g) return fail(SLQ_EINVAL, "slq_kernel_pointgrad_update: accumulator is NULL");
  if (m < 1) return fail(SLQ_EINVAL, "slq_kernel_pointgrad_update: m = %d columns (m >= 1)", m);
  SLQ_TRY(dmat_range(Z, z0, m, g->cross ? "slq_kernel_pointgrad_update(U)" : "slq_kernel_pointgrad_update(Z)"));
  SLQ_TRY(dmat_range(W, w0, m, "slq_kernel_pointgrad_update(W)"));
  if (Z->n != g->nrows || W->n != g->nsum) {
    if (g->cross)
      return fail(SLQ_EINVAL, "slq_kernel_pointgrad_update: the cross form has %lld new points and %lld training points, U %lld rows, W %lld", (long long)g->nrows,
                  (long long)g->nsum, (long long)Z->n, (long long)W->n);
    return fail(SLQ_EINVAL, "slq_kernel_pointgrad_update: the operator has %lld points, Z %lld rows, W %lld", (long long)g->nsum, (long long)Z->n, (long long)W->n);
  }
  if (W->ctx != g->ctx || Z->ctx != g->ctx) return fail(SLQ_EINVAL, "slq_kernel_pointgrad_update: a matrix belongs to another context");
  if (!std::isfinite(alpha) || !std::isfinite(beta)) return fail(SLQ_EINVAL, "slq_kernel_pointgrad_update: alpha = %g, beta = %g must be finite", alpha, beta);
  if (!g->cross) SLQ_TRY(kernel_refuse_scaled(g->op, "slq_kernel_pointgrad_update"));
  HIP_TRY(hipSetDevice(g->ctx->device));
  const slq_operator *op = g->op;
  if (g->cross && g->cross->epoch != op->k_epoch) SLQ_TRY(kernel_cross_rescale(g->cross));  // the hyperparameters have moved: z* follow, before this update
  const KernelPointGradSchedule S = kernel_pointgrad_schedule(g->nrows, g->nsum, g->ctx->num_cus);
  KernelPointGradScale sc;
  for (int k = 0; k < kKernelMaxDim; ++k) sc.ls[k] = op->k_scale->ls[k];
  // training form: P = R(Z, W) + R(W, Z), in this order per chunk; Z and W one matrix and one column range: one pass, twice its weight
  const bool same = !g->cross && Z == W && z0 == w0;
  for (int c0 = 0; c0 < m; c0 += kKernelPointGradCols) {
    const int mc = std::min(kKernelPointGradCols, m - c0);
    const double *Zc = Z->d + (size_t)(z0 + c0) * Z->n, *Wc = W->d + (size_t)(w0 + c0) * W->n;
    SLQ_TRY(kernel_pointgrad_pass(g, S, sc, Zc, Wc, mc, same ? 2.0 * alpha : alpha, c0 == 0 ? beta : 1.0));
    if (!g->cross && !same) SLQ_TRY(kernel_pointgrad_pass(g, S, sc, Wc, Zc, mc, alpha, 1.0));
  }
  g->count += m;
  return SLQ_OK;
}

extern "C" int slq_kernel_pointgrad_get(slq_kernel_pointgrad *g, double *vals, int64_t ld, int64_t *count) {
  if (!g) return fail(SLQ_EINVAL, "slq_kernel_pointgrad_get: accumulator is NULL");
  if (vals && ld < g->d) return fail(SLQ_EINVAL, "slq_kernel_pointgrad_get: ld = %lld is below d = %d", (long long)ld, g->d);
  HIP_TRY(hipSetDevice(g->ctx->device));
  if (vals)
    HIP_TRY(hipMemcpy2DAsync(vals, (size_t)ld * 8, g->vals.p, (size_t)g->d * 8, (size_t)g->d * 8, (size_t)g->nrows, hipMemcpyDeviceToHost, g->ctx->stream));
  HIP_TRY(hipStreamSynchronize(g->ctx->stream));
  if (count) *count = g->count;
  return SLQ_OK;
}

extern "C" int slq_kernel_pointgrad_reset(slq_kernel_pointgrad *g) {
  if (!g) return fail(SLQ_EINVAL, "slq_kernel_pointgrad_reset: accumulator is NULL");
  HIP_TRY(hipSetDevice(g->ctx->device));
  HIP_TRY(hipMemsetAsync(g->vals.p, 0, g->vals_bytes(), g->ctx->stream));
  g->count = 0;
  return SLQ_OK;
}

// kernel_pointgrad_schedule() of slq_kernelpointgrad.hpp as an array: rows per block, row blocks, columns per launch, slabs, tiles per
// slab, then slab_begin[0 .. slabs] (-1 beyond). No HIP call.
extern "C" int slq_debug_kernel_pointgrad_schedule(int64_t nrows, int64_t nsum, int num_cus, int64_t *out, int nout) {
  if (!out || nout < 5 + kKernelCrossMaxSlabs + 1) return fail(SLQ_EINVAL, "slq_debug_kernel_pointgrad_schedule: room for %d values", 5 + kKernelCrossMaxSlabs + 1);
  if (!kernel_extents_ok({nrows, nsum}, num_cus))
    return fail(SLQ_EINVAL, "slq_debug_kernel_pointgrad_schedule: 0 < nrows, nsum < 2^31 - 16 and num_cus positive");
  const KernelPointGradSchedule S = kernel_pointgrad_schedule(nrows, nsum, num_cus);
  kernel_schedule_words({S.rows_per_block, S.nrow_blocks, S.chunk_cols, S.nslabs, S.tiles_per_slab}, S.nslabs, S.slab_begin, kKernelCrossMaxSlabs, out);
  return SLQ_OK;
}

// vals = beta vals + alpha tr(P^-1 dA/dx) = beta vals - alpha sigma^-2 sum_c (L H)_c^T (dA/dx) L_c (tr dA/dx = 0: the diagonal of A does
// not depend on the points), over the columns of the rank reached, 64 at a time through the matrices slq_kernel_precond_trace_grad
// uses: per chunk two column launches and one accumulator update. Everything on the stream; the column count is left as it was.
extern "C" int slq_kernel_precond_trace_pointgrad(slq_operator *op, slq_kernel_pointgrad *g, double alpha, double beta) {
  SLQ_TRY(precond_handle(op, "slq_kernel_precond_trace_pointgrad"));
  if (!g) return fail(SLQ_EINVAL, "slq_kernel_precond_trace_pointgrad: the accumulator is NULL");
  KernelPrecond &pc = *op->pre;
  if (g->cross) return fail(SLQ_EINVAL, "slq_kernel_precond_trace_pointgrad: the accumulator is of the cross form: create it with slq_kernel_pointgrad_create on the base of this preconditioned operator");
  if (g->op != pc.base) return fail(SLQ_EINVAL, "slq_kernel_precond_trace_pointgrad: the accumulator belongs to another operator: create it on the base of this preconditioned operator");
  const int64_t count = g->count;
  SLQ_TRY(precond_trace_columns(op, "slq_kernel_precond_trace_pointgrad", alpha, beta,
                                [&](slq_dmat *Z, slq_dmat *W, int nc, double a, double b) { return slq_kernel_pointgrad_update(g, Z, 0, W, 0, nc, a, b); }));
  g->count = count;
  return SLQ_OK;
}

// the device addresses of L, G, the pivots and the residual diagonal (tests: a refresh keeps them)
extern "C" int slq_debug_kernel_precond_addresses(const slq_operator *op, uint64_t *out4) {
  SLQ_TRY(precond_handle(op, "slq_debug_kernel_precond_addresses"));
  if (!out4) return fail(SLQ_EINVAL, "slq_debug_kernel_precond_addresses: out is NULL");
  const KernelPrecond &pc = *op->pre;
  out4[0] = (uint64_t)(uintptr_t)pc.L.p, out4[1] = (uint64_t)(uintptr_t)pc.G.p, out4[2] = (uint64_t)(uintptr_t)pc.pivots, out4[3] = (uint64_t)(uintptr_t)pc.dres.p;
  return SLQ_OK;
}
// H as the device holds it, rank_max x rank_max row-major (tests: the operand of slq_kernel_precond_columns). Synchronises.
extern "C" int slq_debug_kernel_precond_h(slq_operator *op, double *H) {
  SLQ_TRY(precond_handle(op, "slq_debug_kernel_precond_h"));
  if (!H) return fail(SLQ_EINVAL, "slq_debug_kernel_precond_h: H is NULL");
  const KernelPrecond &pc = *op->pre;
  HIP_TRY(hipSetDevice(op->ctx->device));
  HIP_TRY(hipStreamSynchronize(op->ctx->stream));
  return create_guarded(nullptr, [&]() {
    const size_t r = (size_t)pc.rank_max, rpad = (size_t)pc.rpad;
    std::vector<double> h(rpad * rpad);
    HIP_TRY(hipMemcpy(h.data(), pc.H.p, h.size() * 8, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < r; ++i) std::copy(h.begin() + i * rpad, h.begin() + i * rpad + r, H + i * r);
    return (int)SLQ_OK;
  });
}
// wall time of the last factorisation in ms: {the launches up to the synchronisation, the host part: Jacobi, G and its upload}
extern "C" int slq_debug_kernel_precond_timing(const slq_operator *op, double *out2) {
  SLQ_TRY(precond_handle(op, "slq_debug_kernel_precond_timing"));
  if (!out2) return fail(SLQ_EINVAL, "slq_debug_kernel_precond_timing: out is NULL");
  out2[0] = op->pre->device_ms, out2[1] = op->pre->host_ms;
  return SLQ_OK;
}

extern "C" int slq_measure_stream(slq_context *ctx, int mode, size_t bytes_per_stream, int reps, double *gbps) {
  if (!ctx || !gbps || mode < 0 || mode > 2 || reps < 1 || bytes_per_stream < (1u << 20))
    return fail(SLQ_EINVAL, "bad arguments");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int64_t nvec = (int64_t)(bytes_per_stream / 16);
  double *buf = nullptr;
  HIP_TRY(hipMalloc((void **)&buf, (size_t)nvec * 32 + 64));
  double *w = buf, *q = buf + nvec * 2, *sink = q + nvec * 2;
  hipEvent_t a = nullptr, b = nullptr;
  hipError_t e = hipMemsetAsync(buf, 0, (size_t)nvec * 32 + 64, st);
  if (e == hipSuccess) e = hipEventCreate(&a);
  if (e == hipSuccess) e = hipEventCreate(&b);
  const int blocks = ctx->num_cus * 2;  // the launch shape of the streaming sweeps
  float ms = 0.f;
  if (e == hipSuccess) {
    for (int i = 0; i < 2; ++i) k_stream_probe<<<dim3(blocks), dim3(kBlock), 0, st>>>(w, q, nvec, mode, 1e-9, sink);
    e = hipEventRecord(a, st);
    for (int i = 0; i < reps; ++i) k_stream_probe<<<dim3(blocks), dim3(kBlock), 0, st>>>(w, q, nvec, mode, 1e-9, sink);
    if (e == hipSuccess) e = hipEventRecord(b, st);
    if (e == hipSuccess) e = hipEventSynchronize(b);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, a, b);
    if (e == hipSuccess) e = hipGetLastError();
  }
  if (a) hipEventDestroy(a);
  if (b) hipEventDestroy(b);
  hipFree(buf);
  if (e != hipSuccess) return fail(SLQ_EHIP, "slq_measure_stream: %s", hipGetErrorString(e));
  const double streams = mode == 1 ? 3.0 : 2.0;
  *gbps = streams * (double)nvec * 16.0 * reps / (ms * 1e-3) / 1e9;
  return SLQ_OK;
}

extern "C" int slq_plan_set_probes_device(slq_plan *p, const void *d_X, int64_t ldx) {
  if (!p || !d_X) return fail(SLQ_EINVAL, "plan/X is NULL");
  if (ldx < p->n) return fail(SLQ_EINVAL, "ldx (%lld) < n (%d)", (long long)ldx, p->n);
  HIP_TRY(hipSetDevice(p->ctx->device));
  hipStream_t st = p->ctx->stream;
  if (ldx != p->n) return fail(SLQ_EINVAL, "device probes must be contiguous columns (ldx == n)");
  drop_closing_tail(p);
  if (p->nprobes < p->bpad) HIP_TRY(hipMemsetAsync(slot_ptr(p, 0), 0, (size_t)p->slot_stride * p->esz, st));
  dim3 g((p->n + 63) / 64, (p->nprobes + 63) / 64);
  PROFILED(p, SLQ_K_PROBES, {
    if (p->dtype == SLQ_F64)
      hipLaunchKernelGGL(k_cols_to_panel<double>, g, dim3(256), 0, st, p->n, (const double *)d_X, 0, p->nprobes, (double *)slot_ptr(p, 0), p->PW, p->op->perm_d.as<int32_t>());
    else
      hipLaunchKernelGGL(k_cols_to_panel<float>, g, dim3(256), 0, st, p->n, (const float *)d_X, 0, p->nprobes, (float *)slot_ptr(p, 0), p->PW, p->op->perm_d.as<int32_t>());
  });
  p->pdf_sphere = 0;
  return init_from_probes(p, 0);
}

extern "C" int slq_fttr_batch(slq_context *ctx, int nb, int n, int k, const double *theta, const double *alpha,
                              const double *beta, double *weights) {
  if (!ctx || !theta || !alpha || !beta || !weights) return fail(SLQ_EINVAL, "NULL argument");
  if (nb <= 0 || n <= 0 || k <= 0) return fail(SLQ_EINVAL, "bad sizes");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  double *buf = nullptr;
  const size_t nth = (size_t)nb * k, nab = (size_t)nb * n;
  HIP_TRY(hipMalloc((void **)&buf, (2 * nth + 2 * nab) * 8));
  double *dth = buf, *dw = buf + nth, *da = dw + nth, *db = da + nab;
  hipError_t e = hipMemcpyAsync(dth, theta, nth * 8, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(da, alpha, nab * 8, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(db, beta, nab * 8, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    k_fttr<<<dim3((unsigned)((nth + 127) / 128)), dim3(128), 0, st>>>(nb, n, k, dth, da, db, dw);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(weights, dw, nth * 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  hipFree(buf);
  if (e != hipSuccess) return fail(SLQ_EHIP, "slq_fttr_batch: %s", hipGetErrorString(e));
  return SLQ_OK;
}

extern "C" int slq_eigh_tridiag_batch(slq_context *ctx, int nb, int deg, const double *d, const double *e, double *w,
                                      double *Z) {
  if (!ctx || !d || !e || !w) return fail(SLQ_EINVAL, "ctx/d/e/w is NULL");
  if (nb <= 0 || deg <= 0 || deg > kMaxDeg) return fail(SLQ_EINVAL, "bad batch size or degree (deg <= %d)", kMaxDeg);
  // eigenvectors on chip when they fit in LDS (deg <= 141), otherwise in a global scratch that stays in L2
  const size_t lds_onchip = ((size_t)2 * deg + (size_t)deg * (deg + 1)) * 8 + (size_t)deg * sizeof(int);
  const bool zg = lds_onchip > 160 * 1024;
  const size_t lds = zg ? (size_t)2 * deg * 8 + (size_t)deg * sizeof(int) : lds_onchip;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t in = (size_t)nb * deg, zz = Z ? in * deg : 0, zs = zg ? in * (deg + 1) : 0;
  double *buf = nullptr;
  HIP_TRY(hipMalloc((void **)&buf, (3 * in + zz + zs + 1) * 8));
  double *dd = buf, *de = dd + in, *dw = de + in, *dz = Z ? dw + in : nullptr, *dscr = zg ? dw + in + zz : nullptr;
  int *dfail = (int *)(dw + in + zz + zs);
  hipError_t err = hipMemcpyAsync(dd, d, in * 8, hipMemcpyHostToDevice, st);
  if (err == hipSuccess) err = hipMemcpyAsync(de, e, in * 8, hipMemcpyHostToDevice, st);
  if (err == hipSuccess) err = hipMemsetAsync(dfail, 0, sizeof(int), st);
  if (err == hipSuccess && lds > 48 * 1024)
    err = hipFuncSetAttribute((const void *)k_eigh_tridiag<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (err == hipSuccess) {
    if (zg)
      k_eigh_tridiag<true><<<dim3(nb), dim3(64), lds, st>>>(deg, dd, de, dw, dz, dscr, dfail);
    else
      k_eigh_tridiag<false><<<dim3(nb), dim3(64), lds, st>>>(deg, dd, de, dw, dz, nullptr, dfail);
    err = hipGetLastError();
  }
  int bad = 0;
  if (err == hipSuccess) err = hipMemcpyAsync(&bad, dfail, sizeof(int), hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipMemcpyAsync(w, dw, in * 8, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess && Z) err = hipMemcpyAsync(Z, dz, zz * 8, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  hipFree(buf);
  if (err != hipSuccess) return fail(SLQ_EHIP, "slq_eigh_tridiag_batch: %s", hipGetErrorString(err));
  if (bad) return fail(SLQ_ENOTCONV, "tridiagonal QL did not converge for at least one matrix");
  return SLQ_OK;
}

extern "C" int slq_quadrature_batch(slq_context *ctx, int nb, int deg, const double *d, const double *e,
                                    int fun_id, const double *fun_params, double *quad, double *nodes,
                                    double *weights) {
  if (!ctx || !d || !e) return fail(SLQ_EINVAL, "ctx/d/e is NULL");
  if (nb <= 0 || deg <= 0 || deg > kMaxDeg) return fail(SLQ_EINVAL, "bad batch size or degree");
  if (fun_id < SLQ_FUN_NONE || fun_id > SLQ_FUN_SOFTSIGN) return fail(SLQ_EINVAL, "Unknown function id %d.", fun_id);
  const QuadShape qs = quadrature_shape(deg, nb);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int bp = (nb + 63) / 64 * 64;
  StepState s;
  memset(&s, 0, sizeof(s));
  s.bpad = bp;
  s.nprobes = nb;
  s.deg = deg;
  double *buf = nullptr;
  const size_t in = (size_t)nb * deg;
  const size_t total = (size_t)(2 * (deg + 1) + 1) * bp + 2 * in + bp + 2 * (size_t)bp * deg + 8;
  HIP_TRY(hipMalloc((void **)&buf, total * 8));
  double *q = buf;
  s.alpha = q; q += (size_t)(deg + 1) * bp;
  s.nu = q; q += (size_t)(deg + 1) * bp;
  s.vnorm2 = q; q += bp;
  double *dd = q; q += in;
  double *de = q; q += in;
  double *dq = q; q += bp;
  double *dn = q; q += (size_t)bp * deg;
  double *dw = q; q += (size_t)bp * deg;
  int *dfail = (int *)q;
  int rc = SLQ_OK;
  hipError_t err = hipMemcpyAsync(dd, d, in * 8, hipMemcpyHostToDevice, st);
  if (err == hipSuccess) err = hipMemcpyAsync(de, e, in * 8, hipMemcpyHostToDevice, st);
  if (err == hipSuccess) err = hipMemsetAsync(dfail, 0, sizeof(int), st);
  if (err == hipSuccess) {
    k_load_tridiag<<<dim3((bp + 255) / 256), dim3(256), 0, st>>>(s, dd, de, nb);
    if (qs.lds > 48 * 1024)
      err = hipFuncSetAttribute((const void *)k_quadrature, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  }
  if (err == hipSuccess) {
    const double p0 = fun_params ? fun_params[0] : 0.0, p1 = fun_params ? fun_params[1] : 0.0;
    k_quadrature<<<dim3(qs.grid), dim3(64), qs.lds, st>>>(s, qs.lanes, fun_id, p0, p1, dq, dn, dw, dfail);
    err = hipGetLastError();
  }
  int bad = 0;
  if (err == hipSuccess) err = hipMemcpyAsync(&bad, dfail, sizeof(int), hipMemcpyDeviceToHost, st);
  if (err == hipSuccess && quad) err = hipMemcpyAsync(quad, dq, (size_t)nb * 8, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess && nodes) err = hipMemcpyAsync(nodes, dn, in * 8, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess && weights) err = hipMemcpyAsync(weights, dw, in * 8, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  hipFree(buf);
  if (err != hipSuccess) rc = fail(SLQ_EHIP, "slq_quadrature_batch: %s", hipGetErrorString(err));
  else if (bad) rc = fail(SLQ_ENOTCONV, "tridiagonal QL did not converge for at least one rule");
  return rc;
}

// Gauss-Radau rules of nb given Jacobi matrices (d, e as slq_quadrature_batch; beta_m[i]: the coupling of matrix i to its
// border, the norm of the Lanczos residual after m steps): the stand-alone form of slq_plan_quadrature_at's rule 1.
extern "C" int slq_quadrature_radau_batch(slq_context *ctx, int nb, int m, const double *d, const double *e, const double *beta_m,
                                          double endpoint, int fun_id, const double *fun_params, double *quad, double *nodes,
                                          double *weights) {
  if (!ctx || !d || !e || !beta_m) return fail(SLQ_EINVAL, "ctx/d/e/beta_m is NULL");
  if (nb <= 0 || m <= 0 || m >= kMaxDeg) return fail(SLQ_EINVAL, "bad batch size or degree (m < %d)", kMaxDeg);
  if (!std::isfinite(endpoint)) return fail(SLQ_EINVAL, "slq_quadrature_radau_batch: the endpoint must be finite");
  if (fun_id < SLQ_FUN_NONE || fun_id > SLQ_FUN_SOFTSIGN) return fail(SLQ_EINVAL, "Unknown function id %d.", fun_id);
  const int lanes = quadrature_lanes(m + 1);
  const size_t lds = (size_t)3 * (m + 1) * lanes * 8;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int bp = (nb + 63) / 64 * 64;
  StepState s;
  memset(&s, 0, sizeof(s));
  s.bpad = bp;
  s.nprobes = nb;
  s.deg = m;
  double *buf = nullptr;
  const size_t in = (size_t)nb * m, out = (size_t)nb * (m + 1);
  const size_t total = (size_t)(2 * (m + 1) + 1) * bp + 2 * in + nb + 2 * (size_t)bp + 2 * out + (size_t)bp / 2 + 8;
  HIP_TRY(hipMalloc((void **)&buf, total * 8));
  double *q = buf;
  s.alpha = q; q += (size_t)(m + 1) * bp;
  s.nu = q; q += (size_t)(m + 1) * bp;
  s.vnorm2 = q; q += bp;
  double *dd = q; q += in;
  double *de = q; q += in;
  double *db = q; q += nb;
  double *dq = q; q += bp;
  double *dg = q; q += bp;
  double *dn = q; q += out;
  double *dw = q; q += out;
  s.steps = (int *)q; q += bp / 2;  // (bp ints)
  int *dflags = (int *)q;
  int rc = SLQ_OK;
  hipError_t err = hipMemcpyAsync(dd, d, in * 8, hipMemcpyHostToDevice, st);
  if (err == hipSuccess) err = hipMemcpyAsync(de, e, in * 8, hipMemcpyHostToDevice, st);
  if (err == hipSuccess) err = hipMemcpyAsync(db, beta_m, (size_t)nb * 8, hipMemcpyHostToDevice, st);
  if (err == hipSuccess) err = hipMemsetAsync(dflags, 0, 2 * sizeof(int), st);
  if (err == hipSuccess) {
    k_load_tridiag<<<dim3((bp + 255) / 256), dim3(256), 0, st>>>(s, dd, de, nb);
    k_load_residual<<<dim3((bp + 255) / 256), dim3(256), 0, st>>>(s, db, nb);
    if (lds > 48 * 1024)
      err = hipFuncSetAttribute((const void *)k_quadrature_at, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  }
  if (err == hipSuccess) {
    const double p0 = fun_params ? fun_params[0] : 0.0, p1 = fun_params ? fun_params[1] : 0.0;
    k_quadrature_at<<<dim3((nb + lanes - 1) / lanes), dim3(64), lds, st>>>(s, m, 1, endpoint, 0.0, lanes, fun_id, p0, p1, dq, dg, dn, dw, dflags);
    err = hipGetLastError();
  }
  int flags[2] = {0, 0};
  if (err == hipSuccess) err = hipMemcpyAsync(flags, dflags, 2 * sizeof(int), hipMemcpyDeviceToHost, st);
  if (err == hipSuccess && quad) err = hipMemcpyAsync(quad, dq, (size_t)nb * 8, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess && nodes) err = hipMemcpyAsync(nodes, dn, out * 8, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess && weights) err = hipMemcpyAsync(weights, dw, out * 8, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  hipFree(buf);
  if (err != hipSuccess) rc = fail(SLQ_EHIP, "slq_quadrature_radau_batch: %s", hipGetErrorString(err));
  else if (flags[1]) rc = fail(SLQ_EINVAL, "slq_quadrature_radau_batch: endpoint = %g is not below the smallest eigenvalue of every matrix", endpoint);
  else if (flags[0]) rc = fail(SLQ_ENOTCONV, "tridiagonal QL did not converge for at least one rule");
  return rc;
}

// ---------------------------------------------------------------------------------------------------
// stand-alone operator product
// ---------------------------------------------------------------------------------------------------
extern "C" int slq_operator_matmat(slq_operator *op, const void *X, int64_t ldx, void *Y, int64_t ldy, int b) {
  if (!op || !X || !Y || b <= 0) return fail(SLQ_EINVAL, "bad arguments");
  if (ldx < op->n || ldy < op->n) return fail(SLQ_EINVAL, "leading dimension < n");
  slq_plan *p = nullptr;
  // a keep_basis plan with deg = 1 gives two slots: 0 = X, 1 = Y
  SLQ_TRY(plan_create_mode(op->ctx, op, b, 1, 0, PlanKind::KeepBasis, &p, true));
  hipStream_t st = op->ctx->stream;
  int rc = slq_plan_set_probes(p, X, ldx);
  if (rc == SLQ_OK) {
    if (op->kind == OP_CSR) {
      dim3 g(p->nblkS, p->NP);
      DISPATCH(p->dtype, p->LPR,
               (k_spmm_plain<F, L><<<g, dim3(kBlock), 0, st>>>(p->n, op->csr.rp(), op->csr.ci(),
                                   op->csr.vals.as<const F>(), (const F *)slot_ptr(p, 0), (F *)slot_ptr(p, 1), p->n)));
    } else {
      rc = apply_operator_unfused(p, 0);
      if (rc == SLQ_OK) {
        hipError_t e = hipMemcpyAsync(slot_ptr(p, 1), p->T, (size_t)p->slot_stride * p->esz, hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) rc = fail(SLQ_EHIP, "copy: %s", hipGetErrorString(e));
      }
    }
  }
  if (rc == SLQ_OK) rc = panel_to_host(p, 1, 0, b, Y, ldy, nullptr);
  slq_plan_destroy(p);
  return rc;
}

// ---------------------------------------------------------------------------------------------------
// one-shot entries
// ---------------------------------------------------------------------------------------------------
extern "C" int slq_quad_batch(slq_context *ctx, slq_operator *op, const void *X, int64_t ldx, int pdf,
                              uint64_t seed, uint64_t probe_offset, int nprobes, int deg, double rtol,
                              int orth, int fun_id, const double *fun_params, double *quad_out,
                              double *nodes_out, double *weights_out) {
  if (!ctx || !op) return fail(SLQ_EINVAL, "ctx/op is NULL");
  if (nprobes <= 0) return fail(SLQ_EINVAL, "nprobes must be positive");
  int d = deg, o = orth;
  SLQ_TRY(normalise_params(op->n, &d, &o));
  // size the probe chunk to the free device memory (all probes at once when they fit)
  size_t free_b = 0, total_b = 0;
  SLQ_TRY(slq_context_meminfo(ctx, &free_b, &total_b));
  int chunk = nprobes;
  for (;;) {
    size_t need = 0;
    SLQ_TRY(plan_bytes_on(op, chunk, d, o, 0, &need));
    if (need + ((size_t)1 << 30) <= free_b || chunk <= 8) break;
    chunk = (chunk + 1) / 2;
  }
  int rc = SLQ_OK;
  for (int c0 = 0; c0 < nprobes && rc == SLQ_OK; c0 += chunk) {
    const int nc = std::min(chunk, nprobes - c0);
    slq_plan *p = nullptr;
    rc = slq_plan_create(ctx, op, nc, d, o, 0, &p);
    if (rc != SLQ_OK) break;
    if (X)
      rc = slq_plan_set_probes(p, (const char *)X + (size_t)c0 * (size_t)ldx * esize(op->dtype), ldx);
    else
      rc = slq_plan_generate_probes(p, pdf, seed, probe_offset + (uint64_t)c0);
    if (rc == SLQ_OK) rc = slq_plan_run(p, rtol);
    if (rc == SLQ_OK)
      rc = slq_plan_quadrature(p, fun_id, fun_params, quad_out ? quad_out + c0 : nullptr,
                               nodes_out ? nodes_out + (size_t)c0 * d : nullptr,
                               weights_out ? weights_out + (size_t)c0 * d : nullptr);
    slq_plan_destroy(p);
  }
  return rc;
}

extern "C" int slq_fAv_batch(slq_context *ctx, slq_operator *op, const void *X, int64_t ldx, int nvec, int deg,
                             double rtol, int orth, int fun_id, const double *fun_params, void *Y, int64_t ldy) {
  return slq_fAv_batch_mode(ctx, op, X, ldx, nvec, deg, rtol, orth, fun_id, fun_params, 1, Y, ldy, nullptr);
}

extern "C" int slq_fAv_batch_mode(slq_context *ctx, slq_operator *op, const void *X, int64_t ldx, int nvec, int deg, double rtol, int orth,
                                  int fun_id, const double *fun_params, int basis_mode, void *Y, int64_t ldy, int *basis_used) {
  if (!ctx || !op || !X || !Y) return fail(SLQ_EINVAL, "ctx/op/X/Y is NULL");
  if (basis_mode < 0 || basis_mode > 2) return fail(SLQ_EINVAL, "basis_mode %d (0 automatic, 1 kept basis, 2 recompute)", basis_mode);
  if (nvec <= 0) return fail(SLQ_EINVAL, "nvec must be positive");
  if (ldx < op->n || ldy < op->n) return fail(SLQ_EINVAL, "ldx/ldy < n");
  int d = deg, o = orth;
  SLQ_TRY(normalise_params(op->n, &d, &o));
  // kept basis: the whole basis of every column is kept (deg + 1 panels): chunk the columns to the free device memory.
  // Automatic: the kept basis when the WHOLE column count fits, otherwise recompute plans (whole count first, then halving).
  size_t free_b = 0, total_b = 0;
  SLQ_TRY(slq_context_meminfo(ctx, &free_b, &total_b));
  int mode = basis_mode;
  if (mode == 0) {
    size_t need = 0;
    SLQ_TRY(plan_bytes_on_mode(op, nvec, d, o, 1, &need));
    mode = need + ((size_t)1 << 30) <= free_b ? 1 : 2;
  }
  if (basis_used) *basis_used = mode;
  int chunk = nvec;
  for (;;) {
    size_t need = 0;
    SLQ_TRY(plan_bytes_on_mode(op, chunk, d, o, mode, &need));
    if (need + ((size_t)1 << 30) <= free_b || chunk <= 8) break;
    chunk = (chunk + 1) / 2;
  }
  const size_t es = esize(op->dtype);
  int rc = SLQ_OK;
  slq_plan *p = nullptr;
  int plan_cols = 0;
  for (int c0 = 0; c0 < nvec && rc == SLQ_OK; c0 += chunk) {
    const int nc = std::min(chunk, nvec - c0);
    if (nc != plan_cols) {
      if (p) slq_plan_destroy(p);
      p = nullptr;
      rc = plan_create_mode(ctx, op, nc, d, o, mode == 2 ? PlanKind::Recompute : PlanKind::KeepBasis, &p);
      plan_cols = nc;
      if (rc != SLQ_OK) break;
    }
    rc = slq_plan_set_probes(p, (const char *)X + (size_t)c0 * (size_t)ldx * es, ldx);
    if (rc == SLQ_OK) rc = slq_plan_run(p, rtol);
    if (rc == SLQ_OK) rc = slq_plan_fun_action(p, fun_id, fun_params, (char *)Y + (size_t)c0 * (size_t)ldy * es, ldy);
  }
  if (p) slq_plan_destroy(p);
  return rc;
}

template <typename F>
static int lanczos_single(slq_context *ctx, slq_operator *op, F *v, int deg, F rtol, int orth, F *alpha,
                          F *beta, F *Q, size_t ncv) {
  if (!ctx || !op || !v || !alpha || !beta || !Q) return fail(SLQ_EINVAL, "NULL argument");
  if (op->dtype != (sizeof(F) == 8 ? SLQ_F64 : SLQ_F32)) return fail(SLQ_EINVAL, "operator dtype does not match the entry point");
  if (deg < 1) return fail(SLQ_EINVAL, "Number of steps must be positive!");
  if (deg > op->n) return fail(SLQ_EINVAL, "deg exceeds the operator dimension");
  // precondition of the reference kernel (lanczos.h:91): orth < ncv <= deg is NOT enforced there;
  // what it needs to be well defined is 2 <= ncv and orth <= ncv
  if (ncv < 2 || (size_t)std::max(orth, 0) > ncv) return fail(SLQ_EINVAL, "need ncv >= 2 and orth <= ncv (ncv=%zu, orth=%d)", ncv, orth);
  if (orth < 0) return fail(SLQ_EINVAL, "orth must be non-negative at the native boundary");
  const int n = (int)op->n;
  const bool keep = true;
  slq_plan *p = nullptr;
  SLQ_TRY(slq_plan_create(ctx, op, 1, deg, orth, keep, &p));
  int rc = slq_plan_set_probes(p, v, n);
  // Stale ring columns. The reference clears only column ncv-1 and writes column 0 on entry
  // (lanczos.h:118-120); during the first orth-1 steps its MGS sweep also walks columns ncv-1,
  // ncv-2, ... ncv-orth+1 with whatever the caller left there (lanczos.h:58 with reverse indices),
  // e.g. the previous probe's Lanczos vectors when MatrixFunction.quad reuses its Q
  // (operators.py:138-148). Reproduce that: those columns become vectors t = -1, -2, ... of the
  // ring (t = -1 is the cleared column), with nu_t = ||column||.
  const int nst = (rc == SLQ_OK && p->orth >= 2) ? p->orth - 1 : 0;
  if (nst > 0) {
    hipStream_t st = ctx->stream;
    std::vector<double> norms((size_t)nst + 1, 0.0);
    bool any = false;
    for (int k = 2; k <= nst && rc == SLQ_OK; ++k) {  // t = -k  <->  caller column ncv - k
      const F *col = Q + (size_t)(ncv - k) * n;
      double s2 = 0.0;
      for (int i = 0; i < n; ++i) s2 += (double)col[i] * (double)col[i];
      norms[(size_t)k] = std::sqrt(s2);
      if (s2 > 0.0) any = true;
    }
    if (any) {
      rc = ensure_stage(p, 1);
      for (int k = 1; k <= nst && rc == SLQ_OK; ++k) {
        const int slot = p->S - k;
        hipError_t e = hipMemsetAsync(slot_ptr(p, slot), 0, (size_t)p->slot_stride * p->esz, st);
        if (e == hipSuccess && k >= 2 && norms[(size_t)k] > 0.0) {
          e = hipMemcpyAsync(p->stage, Q + (size_t)(ncv - k) * n, (size_t)n * sizeof(F), hipMemcpyHostToDevice, st);
          if (e == hipSuccess) {
            dim3 g((n + 63) / 64, 1);
            k_cols_to_panel<F><<<g, dim3(256), 0, st>>>(n, (const F *)p->stage, 0, 1, (F *)slot_ptr(p, slot), p->PW, op->perm_d.as<int32_t>());
            e = hipStreamSynchronize(st);
          }
        }
        if (e == hipSuccess) e = hipMemcpyAsync(p->st.nu - (size_t)k * p->bpad, &norms[(size_t)k], sizeof(double), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = fail(SLQ_EHIP, "stale ring upload: %s", hipGetErrorString(e));
      }
      if (rc == SLQ_OK) p->nstale = nst;
    }
  }
  if (rc == SLQ_OK) rc = slq_plan_run(p, (double)rtol);
  std::vector<F> a(deg + 1), b(deg + 1);
  int32_t steps = 0;
  if (rc == SLQ_OK) rc = slq_plan_get_tridiag(p, a.data(), b.data(), &steps);
  if (rc == SLQ_OK) {
    // the reference writes alpha[0..steps) and beta[0..steps]; later entries keep the caller's values
    for (int t = 0; t < steps; ++t) alpha[t] = a[t];
    for (int t = 0; t <= steps; ++t) beta[t] = b[t];
    // ring columns: Lanczos vector t sits in column t % ncv; the last write wins (lanczos.h:143-147).
    // Vectors 0..steps-1 are written (vector `steps` is never normalised into the ring, :140-142).
    std::vector<F> Qfull((size_t)n * deg);
    rc = slq_plan_get_basis(p, 0, Qfull.data(), n);
    if (rc == SLQ_OK) {
      // column ncv-1 is zeroed on entry (lanczos.h:119) unless a later vector lands there
      memset(Q + (size_t)(ncv - 1) * n, 0, (size_t)n * sizeof(F));
      for (int t = 0; t < steps; ++t) memcpy(Q + (size_t)(t % ncv) * n, Qfull.data() + (size_t)t * n, (size_t)n * sizeof(F));
    }
    // v is scratch in the reference and ends as the last unnormalised residual; give it back
    if (rc == SLQ_OK) {
      const int slot = steps % p->S;
      rc = panel_to_host(p, slot, 0, 1, v, n, nullptr);
    }
  }
  slq_plan_destroy(p);
  return rc == SLQ_OK ? steps : rc;
}

extern "C" int slq_lanczos_f64(slq_context *ctx, slq_operator *op, double *v, int deg, double rtol, int orth,
                               double *alpha, double *beta, double *Q, size_t ncv) {
  return lanczos_single<double>(ctx, op, v, deg, rtol, orth, alpha, beta, Q, ncv);
}
extern "C" int slq_lanczos_f32(slq_context *ctx, slq_operator *op, float *v, int deg, float rtol, int orth,
                               float *alpha, float *beta, float *Q, size_t ncv) {
  return lanczos_single<float>(ctx, op, v, deg, rtol, orth, alpha, beta, Q, ncv);
}

#ifdef SLQ_DEBUG_TIMES
// Diagnostic build only (-DSLQ_DEBUG_TIMES, scripts/wave_drift.py): a device buffer of per-wave progress stamps.
static size_t g_dbg_bytes = 0;
extern "C" int slq_debug_times_begin(size_t bytes) {
  if (g_dbg_host_handle) hipFree(g_dbg_host_handle);
  HIP_TRY(hipMalloc((void **)&g_dbg_host_handle, bytes));
  HIP_TRY(hipMemset(g_dbg_host_handle, 0, bytes));
  g_dbg_bytes = bytes;
  HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(slq::g_dbg_times), &g_dbg_host_handle, sizeof(void *)));
  return SLQ_OK;
}
extern "C" int slq_debug_times_read(void *host, size_t bytes) {
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(host, g_dbg_host_handle, std::min(bytes, g_dbg_bytes), hipMemcpyDeviceToHost));
  return SLQ_OK;
}
#endif
