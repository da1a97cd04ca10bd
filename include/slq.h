/* slq.h — C-ABI of the MI355X stochastic-Lanczos-quadrature engine (libslq).
 *
 * This is the drop-in boundary for the reference's native hot path. Plain pointers, sizes and
 * opaque handles only; no C++ or torch types cross it. All entry points return 0 on success or a
 * negative SLQ_E* code (never throw); slq_last_error() gives the message for the calling thread.
 *
 * Reference interfaces replaced (paths relative to the reference repo root):
 *   - primate._lanczos.lanczos(A, v, deg, rtol, orth, alpha, beta, Q)
 *       src/primate/_lanczos.cpp:88-99 (six overloads registered at :102-112)
 *       -> slq_lanczos_f64 / slq_lanczos_f32
 *   - the native kernels behind it, src/primate/include/lanczos.h:43-66 (orth_vector) and
 *       :92-149 (lanczos_recurrence)              -> the plan's device loop (slq_plan_run)
 *   - the operator plugin concept, src/primate/include/linear_operator.h:25-29
 *       (matvec(const F*, F*) + shape())          -> slq_operator (CSR device fast path,
 *       dense, host-callback fallback, GPU-resident device callback;
 *       src/primate/include/eigen_operators.h:17-104, src/primate/include/pylinop.h:16-73)
 *   - the per-probe Python loop of MatrixFunction.quad, src/primate/operators.py:138-151,
 *       with integrate.quadrature (src/primate/integrate.py:57-76) and the LAPACK call in
 *       src/primate/tridiag.py:10-11               -> slq_quad_batch (one call for P probes)
 *   - MatrixFunction._matvec, src/primate/operators.py:102-124 -> slq_fAv_batch / slq_plan_fun_action
 *   - eigh_tridiag / eigvalsh_tridiag, src/primate/tridiag.py:25-62 -> slq_eigh_tridiag_batch
 *   - random.isotropic, src/primate/random.py:22-41,47-80 -> slq_plan_generate_probes
 *   - the spectral-function registry, src/primate/special.py:78-107 -> SLQ_FUN_* ids
 *   - the planned spectral_density (src/primate/__init__.py:10, README.md:22; the measure of
 *       src/primate/integrate.py:30-35)           -> slq_density_*
 *
 * Conventions kept from the reference: alpha/beta have deg+1 entries, beta[0] = 0
 * (lanczos.h:121); rtol is scaled by sqrt(n) (lanczos.h:110); `orth` = number of most recent
 * Lanczos vectors (current one included) to re-orthogonalise against (lanczos.h:135);
 * out-of-range orth (<0 or >deg) means deg (src/primate/operators.py:80); probes are column-major
 * n x P (src/primate/random.py:76); nodes ascending with weights = squared first eigenvector
 * components (integrate.py:63-64).
 */
#ifndef SLQ_H
#define SLQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLQ_VERSION 100

/* ---- status codes --------------------------------------------------------------------------- */
enum {
  SLQ_OK = 0,
  SLQ_EINVAL = -1,   /* invalid argument (maps to Python AssertionError / ValueError)           */
  SLQ_ENOMEM = -2,   /* host or device allocation failed                                         */
  SLQ_EHIP = -3,     /* a HIP runtime call or kernel failed                                      */
  SLQ_ENODEV = -4,   /* no usable gfx950 device                                                  */
  SLQ_ECALLBACK = -5, /* a host-callback operator returned non-zero                              */
  SLQ_ENOTCONV = -6   /* tridiagonal QL did not converge for at least one probe                   */
};

enum { SLQ_F32 = 0, SLQ_F64 = 1 };

/* Spectral functions; ids and parameter meaning follow src/primate/special.py:78-107:
 *   EXP {t}: exp(t x) | SMOOTHSTEP {a,b}: y=clip((x-a)/d,0,1), d=b-a (1 if a==b), 3y^2-2y^3 |
 *   STEP {c, nonnegative}: (|x| or x) < c ? 0 : 1  (numrank = {1e-6, 1}) |
 *   SOFTSIGN {q} | LOG: log(max(x, eps_f64)) | NONE: skip the reduction (nodes/weights only). */
enum {
  SLQ_FUN_IDENTITY = 0,
  SLQ_FUN_ABS = 1,
  SLQ_FUN_SQRT = 2,
  SLQ_FUN_LOG = 3,
  SLQ_FUN_INV = 4,
  SLQ_FUN_EXP = 5,
  SLQ_FUN_SMOOTHSTEP = 6,
  SLQ_FUN_STEP = 7,
  SLQ_FUN_SOFTSIGN = 8,
  SLQ_FUN_NONE = -1
};

/* Probe distributions (src/primate/random.py:12-18). */
enum { SLQ_PDF_RADEMACHER = 0, SLQ_PDF_NORMAL = 1, SLQ_PDF_SPHERE = 2 };

/* Spectral density kernels (slq_density_create): K(x, theta) of the smoothed per-probe measure. */
enum { SLQ_DENSITY_GAUSSIAN = 0, SLQ_DENSITY_LORENTZIAN = 1, SLQ_DENSITY_HISTOGRAM = 2, SLQ_DENSITY_CDF = 3,
       SLQ_DENSITY_CHEBYSHEV = 4 /* from Chebyshev moments (slq_density_update_moments): no smoothing kernel, bw ignored */ };

typedef struct slq_context slq_context;   /* one per (process, GPU): device id + HIP stream      */
typedef struct slq_operator slq_operator; /* a symmetric linear operator resident on that GPU    */
typedef struct slq_plan slq_plan;         /* workspace + state of one batched Lanczos run        */
typedef struct slq_diag slq_diag;         /* device-resident accumulators of the diagonal estimator */
typedef struct slq_dmat slq_dmat;         /* column-major n x m fp64 matrix resident on the device  */
typedef struct slq_density slq_density;   /* device-resident statistics of a spectral density estimate */
typedef struct slq_sddmm slq_sddmm;       /* device-resident values on a CSR pattern, caller's order */

/* Host-callback operator: y = A x on HOST memory (the fallback for arbitrary Python
 * LinearOperators; mirrors PyLinearOperator::matvec, src/primate/include/pylinop.h:32-40).
 * x has ncols entries, y nrows entries, both of the operator's dtype. Return 0 on success. */
typedef int (*slq_matvec_fn)(void *user, const void *x, void *y);
/* Device plugin: Y = A X for ncols columns; d_X, d_Y are DEVICE pointers to column-major n x ncols arrays of
 * the operator dtype (leading dimension n). The callee enqueues its work on `stream` (a hipStream_t), or on
 * any stream provided it has completed or been ordered after/before `stream` when it returns. Nonzero = error. */
typedef int (*slq_matmat_device_fn)(void *user, const void *d_X, void *d_Y, int64_t n, int ncols, void *stream);

/* ---- context -------------------------------------------------------------------------------- */
const char *slq_last_error(void);
int slq_version(void);
int slq_device_count(int *count);
/* device < 0: use the current HIP device. stream == NULL: the context creates its own stream. */
int slq_context_create(int device, void *hip_stream, slq_context **out);
int slq_context_destroy(slq_context *ctx);
int slq_context_synchronize(slq_context *ctx);
/* bytes free / total on the context's device */
int slq_context_meminfo(slq_context *ctx, size_t *free_bytes, size_t *total_bytes);
/* the HIP device ordinal the context is bound to (device = -1 at creation resolves to the current device) */
int slq_context_device(slq_context *ctx, int *device);

/* ---- operators ------------------------------------------------------------------------------ */
/* CSR, int32 indices, host arrays: copied to the device once (the reference copies the matrix
 * at least three times PER PROBE at its FFI, src/primate/_lanczos.cpp:88-93 +
 * src/primate/include/eigen_operators.h:64). */
int slq_csr_create(slq_context *ctx, int dtype, int64_t n, int64_t nnz, const int32_t *rowptr,
                   const int32_t *colind, const void *vals, slq_operator **out);
/* Same, arrays already on the device. The operator is built exactly as by slq_csr_create (validated, reordered, upper
 * triangle, tiles): those decisions are taken on the host, so one copy of the arrays is read back (once), and the caller
 * may free its arrays after the call. */
int slq_csr_create_device(slq_context *ctx, int dtype, int64_t n, int64_t nnz,
                          const int32_t *d_rowptr, const int32_t *d_colind, const void *d_vals,
                          slq_operator **out);
/* Gram operator x -> A^T (A x) of a rectangular CSR matrix A (mrows x ncols, host arrays): the operator Lanczos sees is
 * ncols x ncols (src/primate/include/eigen_operators.h:57-72, SparseEigenLinearOperator<F, true>; unbound in the reference's
 * Python module, src/primate/_lanczos.cpp:104-111). */
int slq_csr_gram_create(slq_context *ctx, int dtype, int64_t mrows, int64_t ncols, int64_t nnz, const int32_t *rowptr,
                        const int32_t *colind, const void *vals, slq_operator **out);
/* Affine operator A + t B of two n x n CSR matrices (eigen_operators.h:106-137, SparseEigenAffineOperator); t = 0 until
 * slq_operator_set_parameter (eigen_operators.h:134-136) changes it. Stored on the union pattern as an ordinary CSR operator. */
int slq_csr_affine_create(slq_context *ctx, int dtype, int64_t n, int64_t nnz_a, const int32_t *rowptr_a, const int32_t *colind_a,
                          const void *vals_a, int64_t nnz_b, const int32_t *rowptr_b, const int32_t *colind_b, const void *vals_b,
                          slq_operator **out);
int slq_operator_set_parameter(slq_operator *op, double t);
/* Matrix-free kernel operator: for n points x_i in d dimensions (row-major n x d, leading dimension ldp >= d,
 * in the operator's dtype), lengthscales l (nls = 1: a scalar that broadcasts, or nls = d: one per dimension), outputscale s
 * and noise sigma2,
 *   z_i = (x_i - mean(x)) / l     rounded to the operator's dtype: the operator is DEFINED on these z
 *   r2_ij = max(0, |z_i|^2 + |z_j|^2 - 2 z_i.z_j), r2_ii = 0 exactly
 *   A = s phi(r2) + sigma2 I,  phi = exp(-r2/2) (SLQ_KERNEL_RBF), exp(-r) (MATERN12), (1 + sqrt3 r) exp(-sqrt3 r) (MATERN32),
 *                                    (1 + sqrt5 r + 5 r2 / 3) exp(-sqrt5 r) (MATERN52), r = sqrt(r2).
 * mean(x) is taken once, at creation: per dimension the sum over the points in row order in double, divided by n. The matrix is
 * never formed: a product evaluates 16 x 16 tiles of it on the matrix cores and the VALU and feeds them to the product with the
 * probe panel out of registers; the operator holds the points, z and |z|^2: O(n d) words (slq_operator_shape reports nnz = n d).
 * The operator is sequenced like a device callback - direct projections, no Gram rows - and its plans replay captured graphs.
 * SLQ_EINVAL names the first bad value: n, d (1 <= d <= 64), ldp, the profile, nls, a lengthscale that is not positive and
 * finite, s likewise, sigma2 < 0 or not finite, the first point (row, coordinate) that is not finite.
 * slq_kernel_create_device: the points are on the context's GPU (they are read back once, for these checks and the mean, and
 *   copied; the caller's array is not referenced after the call).
 * slq_kernel_set_parameters: new l, s, sigma2. It recomputes z, |z|^2 and the two scalars IN PLACE on the context stream: no
 *   allocation, no upload of points, asynchronous. The product kernel reads all of them from device memory, so a plan created
 *   before the call - and the graphs it has captured - computes with the new values from its next run on.
 * slq_kernel_get_parameters: d, the profile, the d lengthscales (nls == d; NULL: not wanted), s, sigma2 as last set.
 * slq_operator_set_parameter (the t of an affine operator) refuses a kernel operator. */
enum { SLQ_KERNEL_RBF = 0, SLQ_KERNEL_MATERN12 = 1, SLQ_KERNEL_MATERN32 = 2, SLQ_KERNEL_MATERN52 = 3 };
int slq_kernel_create(slq_context *ctx, int dtype, int64_t n, int d, const void *points, int64_t ldp, int profile,
                      const double *lengthscales, int nls, double outputscale, double noise, slq_operator **out);
int slq_kernel_create_device(slq_context *ctx, int dtype, int64_t n, int d, const void *d_points, int64_t ldp, int profile,
                             const double *lengthscales, int nls, double outputscale, double noise, slq_operator **out);
int slq_kernel_set_parameters(slq_operator *op, const double *lengthscales, int nls, double outputscale, double noise);
int slq_kernel_get_parameters(const slq_operator *op, int *d, int *profile, double *lengthscales, int nls, double *outputscale, double *noise);
/* Diagnostics (tests). slq_debug_kernel_points: what the product kernel reads, as it is on the device now - z transposed
 * (dpad x npad; dpad = d rounded up to a multiple of 4, npad = n rounded up to a multiple of 16, zeros beyond d and n), |z|^2
 * (npad) and {s, sigma2}, in the operator's dtype; any may be NULL. slq_debug_kernel_schedule: the schedule of one product for a
 * plan of `panels` panels of `panel_width` columns on `num_cus` compute units, without a device: out[0] rows per workgroup,
 * out[1] row blocks, out[2] 16-column tiles per workgroup, out[3] column chunks, out[4] j slabs, out[5 ..] the slabs + 1 bounds
 * of the slabs in [0, n] (then -1); nout >= 22. */
int slq_debug_kernel_points(slq_operator *op, void *zt, void *nrm, void *params);
/* A diagonally scaled kernel operator: with a vector c of n entries, finite and >= 0, given in double and ROUNDED
 * ONCE to the operator's dtype (the operator is defined on the rounded c, as on the rounded z),
 *   A = s diag(c) phi(r2) diag(c) + sigma2 I,     A_ii = s c_i^2 + sigma2 (r2_ii = 0 as before); c_i = 0 makes row i sigma2 e_i^T.
 * Fixed per-point noise K0 + diag(e) is E^{1/2} (D K0 D + I) E^{1/2} with D = diag(e^{-1/2}); the B = I + W^{1/2} K0 W^{1/2} of a Laplace
 * approximation is D K0 D + I with c = W^{1/2}. The scale sits inside the product kernel (k_kernel_panel_scaled: four multiplies per
 * lane and tile on values already in registers, one per output row in the epilogue); c = 1 everywhere gives the bits of the unscaled
 * operator, and an operator without a scale runs the kernels and produces the bits it did before this entry existed.
 * slq_kernel_set_diag_scale: c of n == the operator's n entries, read before the call returns; c == NULL clears the scale. The device
 *   words (npad of them, zeros in the padding) are allocated by the first set and never move: a plan created before the call - and a
 *   graph it captured while the operator was scaled - computes with new VALUES from its next run on. Whether a scale is set is part of a
 *   plan's graph key (scaled and unscaled are different kernels), so setting, changing and clearing are all honoured by live plans.
 *   SLQ_EINVAL names the first bad entry (negative, nan, inf, or not finite in the operator's dtype) or the wrong length.
 * slq_kernel_get_diag_scale: *is_set (may be NULL); c (NULL: not wanted; else n entries, the ROUNDED values, and a scale must be set).
 * slq_debug_kernel_diag_scale: the npad words as the kernel reads them, in the operator's dtype (tests).
 * NOT built for a scaled operator, and refusing with SLQ_EINVAL at every use (not only at creation): slq_kernel_grad_*,
 * slq_kernel_pointgrad_* of the training form, slq_kernel_precond_create / _refresh and every apply, product or plan run on a
 * preconditioned operator whose base is scaled. slq_kernel_cross_*, slq_kernel_feature_* and the cross form of slq_kernel_pointgrad_*
 * are defined on K0's points and profile: they IGNORE the scale, as they ignore the noise. */
int slq_kernel_set_diag_scale(slq_operator *op, const double *c, int64_t n);
int slq_kernel_get_diag_scale(const slq_operator *op, double *c, int64_t n, int *is_set);
int slq_debug_kernel_diag_scale(slq_operator *op, void *c_dev_words);
int slq_debug_kernel_schedule(int64_t n, int panel_width, int panels, int num_cus, int64_t *out, int nout);
/* A Toeplitz operator: A_ij = c[i-j] for i >= j, r[j-i] for j > i (r[0] is ignored, as in SciPy; r == NULL: r = c), with
 * c and r given in double and ROUNDED ONCE to the operator's dtype. The operator is SYMMETRIC iff the rounded r[1:] equals c[1:] bitwise.
 * A product is three FFT passes of length L (the smallest power of two >= 2n) along the rows of the probe panel as it stands in memory: a
 * panel row of PW reals is PW/2 complex numbers, and T real gives T(x1 + i x2) = T x1 + i T x2, so one complex column carries the probes 2q
 * and 2q+1. The symbol FFT_L([c, 0.., r_{n-1} .. r_1]) and every twiddle table are computed on the host in double and uploaded once per set.
 * ERROR: for the output column k of the pair q, |got[:,k] - exact[:,k]|_2 <= eps log2(L) (sum|c| + sum|r[1:]|) |[x_2q, x_2q+1]|_2 - the error
 * of a column is relative to the norm of its PAIR, not of the column (a zero probe next to a large one receives its rounding error).
 * Padding columns of a plan's panel enter every product as zeros. n in [1, 2^22] (L <= 2^23). slq_operator_shape reports nnz = 2n - 1;
 * slq_operator_set_parameter refuses the kind; slq_operator_matmat serves symmetric and non-symmetric operators; EVERY plan creation
 * (slq_plan_create, _recompute, _chebyshev, _chebyshev_action, and the one-shot entries over them) refuses a non-symmetric one.
 * slq_toeplitz_set_values: new c, r of n == the operator's n entries: the symbol is rewritten IN PLACE on the context stream (the call
 *   returns when it is there); plans created before the call, and the graphs they captured, compute with the new values from their next
 *   run. A set that would change the symmetry is refused. SLQ_EINVAL names the first entry that is not finite in the dtype.
 * slq_toeplitz_get_values: the ROUNDED c and r (n entries each; NULL: not wanted) and whether the operator is symmetric.
 * slq_debug_toeplitz_plan (no device): out[0] L, [1] levels (1: one kernel per panel, 2: three, 3: five), [2..4] the pass lengths
 *   (product L; 1 where unused), [5] LDS bytes per workgroup of the largest kernel, [6] complex columns per workgroup, [7] workspace bytes of
 *   a plan (one panel in flight; 0 with one kernel), [8] launches per panel, [9] the largest n supported; nout >= 10.
 * slq_debug_toeplitz_symbol: the symbol the device holds, in natural order and at the scale of FFT_L(e): L complex numbers of the dtype. */
int slq_toeplitz_create(slq_context *ctx, int dtype, int64_t n, const double *c, const double *r, slq_operator **out);
int slq_toeplitz_set_values(slq_operator *op, const double *c, const double *r, int64_t n);
int slq_toeplitz_get_values(const slq_operator *op, double *c, double *r, int64_t n, int *symmetric);
int slq_debug_toeplitz_plan(int64_t n, int dtype, int panel_width, int64_t *out, int nout);
int slq_debug_toeplitz_symbol(slq_operator *op, void *symbol_natural_order);
/* Bytes of device memory the process's operators (and the scratch of operator builds in flight) hold now: back where it was once
 * every operator created since has been destroyed (tests). No HIP call. */
int slq_debug_operator_device_bytes(int64_t *live);
/* Dense symmetric n x n, column-major with leading dimension lda (host array, copied). */
int slq_dense_create(slq_context *ctx, int dtype, int64_t n, const void *A, int64_t lda,
                     slq_operator **out);
/* Host-callback operator (device <-> host round trip per Lanczos step and probe). */
/* A GPU-resident LinearOperator plugin (e.g. a torch module, a user's HIP kernel): the Lanczos vectors never
 * leave HBM. Same place in the reference: any object satisfying the LinearOperator concept
 * (src/primate/include/linear_operator.h:25-29), here with device buffers. */
int slq_device_callback_create(slq_context *ctx, int dtype, int64_t n, slq_matmat_device_fn fn, void *user,
                               slq_operator **out);
int slq_callback_create(slq_context *ctx, int dtype, int64_t n, slq_matvec_fn fn, void *user,
                        slq_operator **out);
int slq_operator_destroy(slq_operator *op);
int slq_operator_shape(const slq_operator *op, int64_t *nrows, int64_t *ncols, int64_t *nnz,
                       int *dtype);
/* Y = A X for a column-major host panel (n x b, ld); exercises the device SpMM on its own. */
int slq_operator_matmat(slq_operator *op, const void *X, int64_t ldx, void *Y, int64_t ldy,
                        int b);

/* ---- plan: batched lock-step Lanczos over P probes --------------------------------------------- */
/* keep_basis != 0 retains all deg Lanczos vectors (ncv = deg, as MatrixFunction fixes it for the
 * f(A)v action, src/primate/operators.py:75-77); otherwise only max(orth,2)(+1) ring slots are
 * resident (ncv = clip(orth, 2, deg), src/primate/lanczos.py:89). */
int slq_plan_create(slq_context *ctx, slq_operator *op, int nprobes, int deg, int orth,
                    int keep_basis, slq_plan **out);
/* A plan for f(A)v by TWO-PASS Lanczos (Borici 2000; Frommer & Simoncini 2008): no basis is kept. Its ring has
 * the slots of a plan without keep_basis plus up to 8 more, so that one accumulation launch consumes up to 8 finished columns,
 * and two panels lie outside the ring: a stash of the probes and the output. At most ring_slots + 10 panels in all,
 * independent of deg. slq_plan_run is pass 1 (the launches of any run). slq_plan_fun_action, slq_plan_fun_action_dmat and
 * slq_diag_update work as on a keep_basis plan, but EACH CALL COSTS ONE FULL RE-RUN: the coefficients come out of T, the probes
 * come back from the stash, and the recurrence is replayed - bit for bit, its sums are taken in a fixed order - while
 * g_t W_t is added into the output as the columns pass through the ring. Afterwards alpha, beta and steps hold the bits of
 * pass 1: slq_plan_quadrature, slq_plan_get_tridiag, slq_density_update work before and after an action.
 * slq_plan_get_basis and slq_plan_run_steps return SLQ_EINVAL on such a plan. Every probe call (slq_plan_set_probes,
 * _set_probes_device, _generate_probes) also copies the probe panel into the stash, device to device (0.9 ms for a 2 GB panel) -
 * also when only quadratures follow: a plan that never takes an action should be an ordinary one. */
int slq_plan_create_recompute(slq_context *ctx, slq_operator *op, int nprobes, int deg, int orth, slq_plan **out);
/* mode: 0 ring only, 1 kept basis, 2 recompute; ring_slots: slots of the ring itself; acc_cols: ring columns one accumulation
 * launch of a recompute plan or of a Chebyshev action plan (mode 0; slq_plan_create_chebyshev_action) consumes (0 for the
 * other kinds). Any output may be NULL. */
int slq_plan_basis_mode(const slq_plan *plan, int *mode, int *ring_slots, int *acc_cols);
/* Byte accounting of a recompute plan's accumulation launches, which do not read a ring column whose coefficient is zero for
 * every probe of a panel (probes past an early stop): columns read and columns offered, summed over launches and panels since
 * the last reset (SLQ_ACC_SKIP=0: read == offered). Synchronises. */
int slq_plan_action_columns(slq_plan *plan, uint64_t *read, uint64_t *offered, int reset);
int slq_plan_destroy(slq_plan *plan);
/* Device bytes this plan holds / would hold. */
int slq_plan_workspace_bytes(const slq_plan *plan, size_t *bytes);
int slq_plan_query_bytes(int dtype, int64_t n, int nprobes, int deg, int orth, int keep_basis,
                         size_t *bytes);
/* ... of a recompute plan: ring, stash and output (host arithmetic only). Independent of deg once deg > 8. */
int slq_plan_query_bytes_recompute(int dtype, int64_t n, int nprobes, int deg, int orth, size_t *bytes);
/* What the plan decided (panel geometry and launch sequence): for byte models and records. */
typedef struct {
  int panel_width;   /* PW: probes per panel row                                                        */
  int panels;        /* NP                                                                              */
  int ring_slots;    /* S                                                                               */
  int sequence;      /* steps with r_j <= 8: 0 store-and-revisit sweeps, 1 fused recompute passes,      */
                     /* 2 fused passes with the intermediate stored (operators without gather locality),  */
                     /* 3 retired: never returned, 4 ring-fed passes with the                               */
                     /* projections taken from Gram rows of the update passes (one gather pass fewer panel reads) */
  int pipelined;     /* dots/update passes use the pipelined row loop                                   */
  int reordered;     /* rows stored in the XCD-aware reverse Cuthill-McKee order                        */
  int upper_alpha;   /* alpha pass walks the upper triangle (exactly symmetric CSR)                     */
  double far_per_row;/* stored nonzeros per row further than 4096 rows from the diagonal                */
  int tiles;         /* fused passes run on LDS workgroup tiles: 0 no, 1 behind barriers, 2 ring-fed (SLQ_TILES) */
  int fused_alpha;   /* retired: always 0 (kept so that the struct's layout does not change)             */
} slq_plan_info;
int slq_plan_describe(const slq_plan *plan, slq_plan_info *out);

/* Parity mode: host probes, column-major n x nprobes of the plan's dtype (ld >= n). */
int slq_plan_set_probes(slq_plan *plan, const void *X, int64_t ldx);
/* Same, probes already on the device (column-major n x nprobes, contiguous: ldx == n), on the
 * context's stream: nothing crosses PCIe. */
int slq_plan_set_probes_device(slq_plan *plan, const void *d_X, int64_t ldx);
/* Throughput mode: counter-based Philox4x32-10 on the device; the stream of probe `i` depends
 * only on (seed, probe_offset + i), so results do not depend on how probes are sharded. */
int slq_plan_generate_probes(slq_plan *plan, int pdf, uint64_t seed, uint64_t probe_offset);
/* Copy the current probes back as a column-major n x nprobes host panel. */
int slq_plan_get_probes(slq_plan *plan, void *X, int64_t ldx);

/* deg Lanczos steps for all probes (asynchronous on the context stream). Without keep_basis the
 * residual slot deg % S holds no defined value after the run: the last step need not store W_deg. */
int slq_plan_run(slq_plan *plan, double rtol);
/* Resumable form: runs steps [cur, upto), cur = the number of steps done since the probes were set or generated (0
 * then). cur < upto <= deg, else SLQ_EINVAL; rtol must equal the one the run began with. The launches are those of
 * slq_plan_run: slq_plan_run_steps(p, rtol, deg) on fresh probes IS slq_plan_run(p, rtol), and the Jacobi matrix after m
 * steps is the one a plan of degree m, orth min(orth, m) produces. Between two stages (0 < cur < deg) the entries that
 * mean "the finished run" (slq_plan_quadrature, slq_plan_fun_action*, slq_plan_get_basis, slq_diag_update,
 * slq_density_update) return SLQ_EINVAL - use slq_plan_quadrature_at -, and slq_plan_get_tridiag returns the prefix
 * (zeros beyond it). Plans with stale ring columns (the drop-in slq_lanczos_* path) are not resumable. */
int slq_plan_run_steps(slq_plan *plan, double rtol, int upto);
int slq_plan_steps_done(const slq_plan *plan, int *cur);
/* alpha, beta: nprobes x (deg+1) row-major of the plan dtype; steps: nprobes ints. Any may be
 * NULL. Synchronises.
 * beta_deg of a plan without a kept basis is computed at its first request: a run that reaches deg leaves out the update
 * pass of its last step, which stores no vector and whose scalars no quadrature reads (the closing tail; SLQ_LAST_STORE=2 keeps it in the run,
 * slq_plan_closing_state), and this call launches it on the plan's stream before it copies. The numbers are those of a
 * run that launched it at once, bit for bit: nothing the pass reads can change in between (new probes drop it; plans of an
 * affine operator, whose values slq_operator_set_parameter rewrites, never leave it out). */
int slq_plan_get_tridiag(slq_plan *plan, void *alpha, void *beta, int32_t *steps);
/* The closing tail of a plan: the update pass of step deg - 1 and the scalar kernel behind it. *lazy: runs of this plan
 * leave it out (plain quadrature plans whose last update pass stores nothing, on operators with fixed values - not the
 * affine A + t B -, unless created under SLQ_LAST_STORE=2); *pending: the last
 * run left it out and nothing has asked for it yet. slq_plan_get_tridiag, slq_plan_quadrature_at with the Gauss-Radau
 * rule at m = deg and the slq_plan_window_* diagnostics launch a pending tail first; slq_plan_quadrature,
 * slq_density_update, slq_plan_describe and slq_plan_profile_read never do; new probes and slq_plan_destroy drop it
 * without a launch. Either pointer may be NULL. No device work. */
int slq_plan_closing_state(slq_plan *plan, int *lazy, int *pending);
/* Gauss quadrature of every probe's Jacobi matrix on the device, then
 * quad[i] = sum_k f(nodes[i,k]) * weights[i,k] * ||v_i||^2 (src/primate/operators.py:149-150).
 * quad: nprobes doubles or NULL; nodes/weights: nprobes x deg row-major doubles or NULL.
 * Synchronises. */
int slq_plan_quadrature(slq_plan *plan, int fun_id, const double *fun_params, double *quad,
                        double *nodes, double *weights);
/* Quadrature of the first m <= cur steps. rule 0: the m-point Gauss rule (for m = deg after a full run: what
 * slq_plan_quadrature returns, bit for bit). rule 1: the (m+1)-point Gauss-Radau rule with a prescribed node at
 * `endpoint` <= lambda_min(A) (Golub 1973); with the Gauss rule it brackets v^T f(A) v for every f whose derivatives
 * keep one sign (log, inverse, exp(-t x), powers). nodes / weights: nprobes x (m + rule) row-major doubles or NULL. A
 * probe that stopped at or before step m has an exact Gauss rule: its Radau value is its Gauss value (returned as the
 * Gauss rule behind a zero-weight node at the endpoint). An endpoint that is not below the smallest Ritz value of every
 * probe is SLQ_EINVAL. stage (4 doubles or NULL) = {sum_i quad_i, sum_i quad_i^2, sum_i |quad_i - gauss_i| (0 for rule
 * 0), nprobes}, reduced on the device in a fixed order (identical runs give identical bits). Synchronises. */
int slq_plan_quadrature_at(slq_plan *plan, int m, int rule, double endpoint, int fun_id, const double *fun_params,
                           double *quad, double *nodes, double *weights, double *stage);
/* Lanczos basis of probe `probe` as a column-major n x deg host array (normalised columns;
 * columns past an early stop are zero). Requires keep_basis. */
int slq_plan_get_basis(slq_plan *plan, int probe, void *Q, int64_t ldq);
/* Y[:, i] = f(A) x_i ~= ||x_i|| Q_i Y_i (f(theta_i) * Y_i[0,:])  (src/primate/operators.py:113-124);
 * column-major n x nprobes host output. Requires a completed run on a keep_basis plan or on a recompute plan (there
 * every call replays the run: slq_plan_create_recompute). */
int slq_plan_fun_action(slq_plan *plan, int fun_id, const double *fun_params, void *Y,
                        int64_t ldy);

/* Stand-alone Gauss quadrature of nb Jacobi matrices on the device (the C-ABI form of
 * integrate.quadrature(d, e, deg, quad="gw"), src/primate/integrate.py:57-64): d, e are
 * nb x deg row-major doubles, e[:,0] is ignored (must be 0 in the reference, integrate.py:59) and
 * e[:,i] couples i-1 and i. quad[i] = sum_k f(nodes[i,k]) weights[i,k]. Any output may be NULL. */
int slq_quadrature_batch(slq_context *ctx, int nb, int deg, const double *d, const double *e,
                         int fun_id, const double *fun_params, double *quad, double *nodes,
                         double *weights);

/* Stand-alone Gauss-Radau rules of nb Jacobi matrices of size m (d, e as above; beta_m: nb doubles, the coupling of each
 * matrix to its border = the norm of the Lanczos residual after m steps; beta_m[i] = 0: the Gauss rule behind a
 * zero-weight node). nodes / weights: nb x (m+1) row-major doubles or NULL; quad[i] = sum_k f(nodes[i,k]) weights[i,k]. */
int slq_quadrature_radau_batch(slq_context *ctx, int nb, int m, const double *d, const double *e, const double *beta_m,
                               double endpoint, int fun_id, const double *fun_params, double *quad, double *nodes,
                               double *weights);

/* Full eigendecomposition of nb symmetric tridiagonals (eigh_tridiag / eigvalsh_tridiag,
 * src/primate/tridiag.py:25-62; what rayleigh_ritz and MatrixFunction._matvec call): d, e as above
 * (e[:,0] ignored). w: nb x deg ascending eigenvalues. Z: nb x deg x deg row-major, eigenvectors in the
 * COLUMNS of each matrix, or NULL for eigenvalues only. deg <= 512 (eigenvectors on chip up to 141). */
int slq_eigh_tridiag_batch(slq_context *ctx, int nb, int deg, const double *d, const double *e, double *w, double *Z);

/* Tall-skinny dense algebra for the exchangeable estimators (xtrace / hutch++: the host-side
 * np.linalg.qr, Q.T @ W, Z.T @ W, ... of src/primate/trace.py:160-176,199-227,296-302) on the matrix
 * cores (fp64 MFMA). Matrices are column-major n x cols with leading dimension n.
 *   gemm_tn: C (ma x mb, row-major, host) = A[:, a0:a0+ma]^T  B[:, b0:b0+mb]
 *   gemm_nn: OUT[:, o0:o0+mb] = beta * OUT[:, o0:o0+mb] + alpha * A[:, a0:a0+ma] * C  (C: ma x mb row-major host)
 *   slq_plan_fun_action_dmat: f(A) X of a completed keep_basis run straight into OUT's columns;
 *   slq_dmat_ptr + slq_plan_set_probes_device feed a matrix's columns back in as probes. */
int slq_dmat_create(slq_context *ctx, int64_t n, int cols, slq_dmat **out);
int slq_dmat_destroy(slq_dmat *m);
int slq_dmat_set(slq_dmat *m, int c0, int nc, const double *host, int64_t ld);
int slq_dmat_get(slq_dmat *m, int c0, int nc, double *host, int64_t ld);
int slq_dmat_ptr(slq_dmat *m, int c0, void **dptr);
/* Isotropic probes straight into columns [c0, c0+nc): element (seed, probe id = probe_offset + column, row) of
 * the same Philox stream as slq_plan_generate_probes; sphere columns have norm sqrt(n). The batch filler of
 * src/primate/random.py:100-142 (class Isotropic) without a host array. */
int slq_dmat_generate(slq_dmat *m, int c0, int nc, int pdf, uint64_t seed, uint64_t probe_offset);
int slq_dmat_copy(slq_dmat *dst, int d0, slq_dmat *src, int s0, int nc); /* dst[:, d0:d0+nc] = src[:, s0:s0+nc], on the device */
/* dst[dr0:dr0+nrows, d0:d0+nc] = src[sr0:sr0+nrows, s0:s0+nc] between matrices of different heights (device to device): how a
 * row-sharded sketch takes its rows out of full columns and back (xtrace with row-sharded sketches: trace.py:296-302 at scale) */
int slq_dmat_copy_rows(slq_dmat *dst, int d0, int64_t dr0, slq_dmat *src, int s0, int64_t sr0, int64_t nrows, int nc);
int slq_dmat_gemm_tn(slq_dmat *A, int a0, int ma, slq_dmat *B, int b0, int mb, double *C_host);
int slq_dmat_gemm_nn(slq_dmat *OUT, int o0, slq_dmat *A, int a0, int ma, const double *C_host, int mb,
                     double alpha, double beta);
int slq_plan_fun_action_dmat(slq_plan *plan, int fun_id, const double *fun_params, slq_dmat *OUT, int o0);
/* The plan's current probes (set or device-generated, not yet consumed by a run), as the estimators use
 * them (sphere draws scaled to norm sqrt(n), src/primate/random.py:36-41), into OUT's columns
 * [o0, o0 + nprobes): lets xtrace keep its sample matrix W on the device without a host draw. */
int slq_plan_get_probes_dmat(slq_plan *plan, slq_dmat *OUT, int o0);

/* Device bandwidth probe with the access shape of the sweeps (16 B/lane, one contiguous window):
 * mode 0 = two read streams, 1 = in-place triad (2 reads + 1 write), 2 = copy. Reports GB/s. Used by
 * bench.py to quote the roofline fraction against the measured rate as well as the 8 TB/s spec. */
int slq_measure_stream(slq_context *ctx, int mode, size_t bytes_per_stream, int reps, double *gbps);

/* FTTR quadrature weights on the device (integrate.quadrature(..., quad="fttr"),
 * src/primate/integrate.py:65-69 -> src/primate/fttr.py:17-29): theta, weights are nb x k row-major;
 * alpha, beta nb x n row-major (beta[:,0] unused); values as the reference's fttr() returns them. */
int slq_fttr_batch(slq_context *ctx, int nb, int n, int k, const double *theta, const double *alpha,
                   const double *beta, double *weights);

/* Diagonal estimator (the loop body of diag(), src/primate/diagonal.py:74-79): for every probe of a
 * completed keep_basis run, in order, numer += f(A)v * v, denom += v*v, and the running mean of
 * numer/denom (the reference's estimate). Everything stays on the device between updates. */
int slq_diag_create(slq_context *ctx, int64_t n, slq_diag **out);
int slq_diag_destroy(slq_diag *d);
int slq_diag_update(slq_diag *d, slq_plan *plan, int fun_id, const double *fun_params);
/* any of numer / denom / running_mean (n doubles each) and count may be NULL */
int slq_diag_get(slq_diag *d, double *numer, double *denom, double *running_mean, int64_t *count);

/* Spectral density of stochastic Lanczos quadrature (the reference plans it but does not ship it: the commented-out
 * `from .integrate import spectral_density`, src/primate/__init__.py:10, and README.md:22, after Lin, Saad, Yang,
 * SIAM Review 2016). Every probe's Gauss rule is a discrete form of the per-probe measure
 * psi(x; A, v) = sum_i |u_i^T v|^2 delta(x - lambda_i) (src/primate/integrate.py:30-35); an update evaluates
 *   phi_p(x_g) = ||v_p||^2 sum_k tau_pk K(x_g, theta_pk)
 * for every probe p of a completed run and grid point g, and folds the values into per-point running (count, mean,
 * M2) in probe order with the batch-Welford formula (no float atomics: identical runs give identical bits). Kinds:
 *   GAUSSIAN    exp(-(x-theta)^2 / 2 bw^2) / (bw sqrt(2 pi))    ngrid points
 *   LORENTZIAN  (bw / pi) / ((x-theta)^2 + bw^2)                  ngrid points
 *   HISTOGRAM   1[e_g <= theta < e_{g+1}]                         ngrid bins, grid holds ngrid + 1 edges
 *   CDF         1[theta < x]                                      ngrid thresholds
 * grid must be strictly increasing; bw > 0 for the two smooth kinds (ignored otherwise). outside[0] / [1]: the mean
 * node mass below x_0 / above x_{ngrid-1} (theta >= the last edge for HISTOGRAM), so that a grid that misses part of
 * the spectrum shows it. Zero-weight nodes of an early stop add nothing.
 * slq_density_update is asynchronous on the context stream; it runs the QL of the plan's Jacobi matrices only if
 * slq_plan_quadrature has not already done so for this run (and a later slq_plan_quadrature reuses the rule). QL
 * non-convergence (SLQ_ENOTCONV) and a ring-pass bail-out (SLQ_EHIP) are reported by slq_density_get, which
 * synchronises. mean, m2: ngrid doubles each; any output may be NULL. */
int slq_density_create(slq_context *ctx, int kind, int ngrid, const double *grid, double bw, slq_density **out);
int slq_density_update(slq_density *d, slq_plan *plan);
int slq_density_get(slq_density *d, double *mean, double *m2, double *outside, int64_t *count);
int slq_density_destroy(slq_density *d);

/* ---- Chebyshev moments: the kernel polynomial method (Weisse, Wellein, Alvermann, Fehske, Rev. Mod. Phys. 2006; the other
 * method of Lin, Saad, Yang 2016) -------------------------------------------------------------------------------------
 * mu_k = v^T T_k(A~) v with A~ = (A - center) / halfwidth, for every probe of a batch, by the recurrence
 *   w_0 = v, w_1 = A~ v, w_{j+1} = 2 A~ w_j - w_{j-1}
 * and the doubling identities mu_{2j+2} = 2 ||w_{j+1}||^2 - mu_0, mu_{2j+1} = 2 w_{j+1}.w_j - mu_1: nsteps steps give the
 * 2 nsteps + 1 moments mu_0 .. mu_{2 nsteps}, the polynomial degree per product of a Gauss rule. A step is ONE update pass of
 * the orth-0 Lanczos step with constant coefficients (no alpha pass, no orthogonality, no eigensolve) and one scalar kernel,
 * so nsteps is bounded by 16384, not by the Lanczos cap of 512.
 * slq_plan_create_chebyshev: a plan of orth-0 geometry (two ring slots) that holds the moments on the device. The probe
 *   entries, slq_plan_describe, _workspace_bytes, _profile_* and _destroy work on it unchanged; every Lanczos entry
 *   (slq_plan_run, _run_steps, _get_tridiag, _quadrature*, _get_basis, _fun_action*, slq_diag_update, slq_density_update)
 *   returns SLQ_EINVAL, as the entries below do on any other plan.
 * slq_plan_run_chebyshev: enqueues the nsteps steps on the context stream (asynchronous; it consumes the probes like
 *   slq_plan_run). [center - halfwidth, center + halfwidth] must contain the spectrum: where it does not, T_k grows and
 *   |mu_k| > (1 + outside_tol) mu_0 raises the probe's `outside` flag (outside_tol <= 0: the default, 1e-3).
 * slq_plan_get_moments: mu row-major nprobes x (2 nsteps + 1), outside nprobes ints (or NULL). Synchronises. The numbers are
 *   returned (finite or not) whatever the flags say.
 * slq_plan_moment_sum: quad_i = sum_{k < ncoef} coef_k mu_ik, k ascending, ncoef <= 2 nsteps + 1 - with the Chebyshev
 *   coefficients of f on the interval, v_i^T f(A) v_i. quad: nprobes doubles or NULL; stage: the four doubles of
 *   slq_plan_quadrature_at {sum quad, sum quad^2, 0, nprobes} or NULL. SLQ_EINVAL, naming the bounds, if a flag is up.
 * slq_density_update_moments (kind SLQ_DENSITY_CHEBYSHEV only; slq_density_update returns SLQ_EINVAL on that kind): folds
 *   rho_p(x_g) = [g_0 mu_0 + 2 sum_{k>=1} g_k mu_k T_k(x~_g)] / (pi h sqrt(1 - x~_g^2)), x~ = (x - center) / h,
 *   over the first nweights moments with damping factors damp (NULL: all ones; Jackson factors make rho >= 0) into the
 *   accumulator; the integral over the interval is mu_0 = ||v||^2 (the eigenvalue-count normalisation of the other kinds).
 *   Every grid point must lie strictly inside (center - h, center + h). The two `outside` columns are 0. */
int slq_plan_create_chebyshev(slq_context *ctx, slq_operator *op, int nprobes, int nsteps, slq_plan **out);
int slq_plan_run_chebyshev(slq_plan *plan, double center, double halfwidth, double outside_tol);
int slq_plan_get_moments(slq_plan *plan, double *mu, int *outside);
int slq_plan_moment_sum(slq_plan *plan, int ncoef, const double *coef, double *quad, double *stage);
int slq_density_update_moments(slq_density *d, slq_plan *plan, int nweights, const double *damp);

/* ---- The Chebyshev action Y = p(A) X, p(x) = sum_{k <= nsteps} c_k T_k((x - center) / halfwidth) ----------
 * The same polynomial for every column: exactly linear in X and symmetric, one run, no replay, nsteps up to 16384, and the
 * moments and `outside` flags of that run besides. Y = sum_k c_k w_k is summed while the w_k pass through the ring, by one
 * accumulation launch per 16 finished columns (slq_plan_basis_mode's acc_cols).
 * slq_plan_create_chebyshev_action (beside slq_plan_create_chebyshev, which is unchanged: two ring slots, no store in the last
 *   step): a Chebyshev plan whose ring has min(acc_cols, nsteps + 1) slots (2 at least), with ONE output panel behind it -
 *   AT MOST acc_cols + 1 = 17 PANELS in all, whatever nsteps is (the recompute plan's contract: ring_slots + 10). The probes
 *   are ring column 0: no stash. Every step stores its vector. Every Chebyshev entry works on it - slq_plan_run_chebyshev,
 *   _get_moments, _moment_sum, slq_density_update_moments give the bits a plain plan gives -, so one plan serves the quadratic
 *   forms and the action; every Lanczos entry returns SLQ_EINVAL as on any Chebyshev plan.
 * slq_plan_chebyshev_action (beside slq_plan_fun_action): runs the nsteps steps of slq_plan_run_chebyshev with the
 *   accumulation launches in between (class SLQ_K_COMBINE), then copies the output panel to the column-major n x nprobes Y
 *   (ldy >= n). coef: ncoef = nsteps + 1 finite doubles, rounded to the plan's dtype once on the device; a column whose
 *   coefficient is exactly 0.0 is not read (SLQ_ACC_SKIP=0 reads it: the same bits). It consumes the probes and leaves the
 *   moments and flags as a plain run does. Synchronises.
 * slq_plan_chebyshev_action_dmat (beside slq_plan_fun_action_dmat): the same into OUT[:, o0 : o0 + nprobes] (fp64 plans).
 * SLQ_EINVAL, the message naming the cause, and Y / OUT not written: not an action plan (a plain Chebyshev plan, a Lanczos
 *   plan); probes not ready; ncoef != nsteps + 1; a non-finite coefficient; ldy < n; an `outside` flag up after the run (the
 *   message of slq_plan_moment_sum, naming the bounds); and probes that the last probe call DREW ON THE DEVICE FROM THE SPHERE
 *   (slq_plan_generate_probes, SLQ_PDF_SPHERE): their panel holds the normal draw g while the probe is sqrt(n) g / ||g|| - the
 *   moments carry that ratio, the vectors of the ring do not. Draw them on the host and use slq_plan_set_probes.
 * slq_plan_action_columns reports these launches too: whole ring columns read against columns offered (nsteps + 1 per
 *   action), counted once per launch on the host - the mask is the host's and the same for every panel. */
int slq_plan_create_chebyshev_action(slq_context *ctx, slq_operator *op, int nprobes, int nsteps, slq_plan **out);
int slq_plan_chebyshev_action(slq_plan *plan, double center, double halfwidth, double outside_tol, int ncoef, const double *coef,
                              void *Y, int64_t ldy);
int slq_plan_chebyshev_action_dmat(slq_plan *plan, double center, double halfwidth, double outside_tol, int ncoef, const double *coef,
                                   slq_dmat *OUT, int o0);

/* ---- The sampled dense-dense product on a CSR pattern (SDDMM) ----------------------------------------------
 * For symmetric A, d tr f(A) / dA = f'(A), and its Hutchinson estimate on the stored nonzeros e = (row, col) is
 *   G[e] = (1/N) sum_i (f'(A) v_i)[row(e)] v_i[col(e)]
 * - both factors are columns of a slq_dmat already (slq_plan_fun_action_dmat or slq_plan_chebyshev_action_dmat, and
 * slq_plan_get_probes_dmat). A slq_sddmm holds one double per stored nonzero on the device and folds such products in.
 * slq_sddmm_create: the pattern is ANY CSR over n rows and n columns, given as host arrays (copied). It is kept in the caller's
 *   order - never reordered, sorted or deduplicated; a duplicate entry gets its own (equal) value - and it is independent of any
 *   slq_operator: a dense or plugin operator can have a gradient on a pattern of the user's choice. It is validated on the host:
 *   rowptr[0] == 0, rowptr non-decreasing, rowptr[n] == nnz, 0 <= colind < n; SLQ_EINVAL names the first offending row. nnz == 0
 *   is legal (no update launches anything). The values start at 0.
 * slq_sddmm_create_device: the same from arrays on the context's GPU: they are read back once, validated, and the validated
 *   copy is what the kernel reads (as slq_csr_create_device reads its index arrays); the caller's arrays are not referenced
 *   after the call.
 * slq_sddmm_update: vals[e] = beta * vals[e] + alpha * sum_{j < m} W[row(e), w0 + j] * Z[col(e), z0 + j]; with symmetric != 0
 *   the summand is 0.5 * (W[r, .] Z[c, .] + Z[r, .] W[c, .]) - the symmetric part, what a symmetric A can see of its gradient.
 *   beta == 0 does not read the old values. Asynchronous on the context stream; count += m. Every stored nonzero is owned by
 *   one lane (one lane of a wave of its own for a row of more than 64 nonzeros) that sums j ascending: no float atomics, and
 *   identical calls give identical bits. W may be Z. SLQ_EINVAL, the values untouched: a column range outside its matrix, a
 *   matrix that has not n rows, an object of another context, a non-finite alpha or beta.
 * slq_sddmm_get: the nnz values in the caller's order and the columns folded in so far (either may be NULL). Synchronises.
 * slq_sddmm_ptr: the device address of the values, for zero-copy consumers (valid until slq_sddmm_destroy; order reads after
 *   the context stream). slq_sddmm_reset: values and count back to 0 (asynchronous). */
int slq_sddmm_create(slq_context *ctx, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colind, slq_sddmm **out);
int slq_sddmm_create_device(slq_context *ctx, int64_t n, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_colind, slq_sddmm **out);
int slq_sddmm_update(slq_sddmm *s, slq_dmat *W, int w0, slq_dmat *Z, int z0, int m, double alpha, double beta, int symmetric);
int slq_sddmm_get(slq_sddmm *s, double *vals, int64_t *count);
int slq_sddmm_ptr(slq_sddmm *s, void **d_vals);
int slq_sddmm_reset(slq_sddmm *s);
int slq_sddmm_destroy(slq_sddmm *s);
/* The work items an update over this pattern launches, one wave each, as the library cuts them, without a device
 * (csrc/slq_sddmm.hpp: sddmm_schedule). Item i owns the stored nonzeros [e0[i], e1[i]) of the rows row0[i] .. row0[i] + nrows[i]
 * - 1; kind[i] = 0: at most 64 consecutive rows of at most 64 nonzeros, one lane per row; 1: one longer row, the lanes over
 * its nonzeros. The first cap items are written (any array may be NULL); *nitems their number; info (4 values or NULL):
 * workgroups, long rows, the long-row threshold, waves per workgroup. rowptr: n + 1 non-decreasing offsets from 0, else
 * SLQ_EINVAL. No HIP call. */
int slq_debug_sddmm_schedule(int64_t n, const int32_t *rowptr, int32_t *row0, int32_t *nrows, int32_t *kind, int64_t *e0, int64_t *e1,
                             int64_t cap, int64_t *nitems, int64_t *info);

/* ---- Hyperparameter gradients of the kernel operator -------------------------------------------------------
 * For A = s phi(r2) + sigma2 I of slq_kernel_create (d dimensions) and columns of two device matrices Z, W, with
 * C_ij = sum_c Z_ic W_jc, D_ijk = z_ik - z_jk on the operator's rounded z and chi = -2 dphi/dr2 (rbf exp(-r2/2); matern12
 * exp(-r)/r, DEFINED 0 at r2 = 0; matern32 3 exp(-sqrt3 r); matern52 (5/3)(1 + sqrt5 r) exp(-sqrt5 r)), an update computes
 *   g_l[k]   = (s / l_k) sum_ij C_ij chi(r2_ij) D_ijk^2      = sum_c Z_c^T (dA/dl_k) W_c,   k < d
 *   g_s      =           sum_ij C_ij phi(r2_ij)
 *   g_sigma2 =           sum_i  C_ii
 * with r2_ij the operator's own value (its bits, its clamp, 0 on the diagonal). W = probes, Z = f'(A) probes, alpha = 1/N: the
 * Girard-Hutchinson estimate of d tr f(A) / d theta; Z = W = A^-1 y: the gradient of y^T A^-1 y up to its sign. Nothing of size
 * n^2 is held and nothing of size n leaves the device.
 * slq_kernel_grad_create: op must be a kernel operator in fp64 (SLQ_EINVAL names the kind or the dtype otherwise) of ctx. The
 *   accumulator reads op at every update and does not own it: destroy the accumulator first. The d + 2 values start at 0.
 * slq_kernel_grad_update: vals = beta * vals + alpha * (the d + 2 sums over columns [z0, z0 + m) of Z and [w0, w0 + m) of W);
 *   count += m. Columns go 64 to a launch; the chunks of a wider m fold in one after the other. Asynchronous on the context
 *   stream; no atomics: identical calls give identical bits. beta == 0 does not read the old values. It reads the operator's
 *   parameters as they are at the call: a slq_kernel_set_parameters between two updates is honoured by the second, and values
 *   accumulated across such a change mix two operators. SLQ_EINVAL, the values untouched: a NULL handle, a column range outside
 *   its matrix, m < 1, a matrix that has not n rows, an object of another context, a non-finite alpha or beta.
 * slq_kernel_grad_get: nvals == d + 2: [0, d) the lengthscales, ALWAYS per dimension (a scalar lengthscale's gradient is their
 *   sum), [d] the outputscale, [d + 1] the noise; the columns folded in so far (either may be NULL). Synchronises.
 * slq_kernel_grad_reset: values and count back to 0 (asynchronous).
 * Not built for an operator with a diagonal scale (slq_kernel_set_diag_scale): create and every update refuse it with SLQ_EINVAL. */
typedef struct slq_kernel_grad slq_kernel_grad;
int slq_kernel_grad_create(slq_context *ctx, slq_operator *op, slq_kernel_grad **out);
int slq_kernel_grad_update(slq_kernel_grad *g, slq_dmat *Z, int z0, slq_dmat *W, int w0, int m, double alpha, double beta);
int slq_kernel_grad_get(slq_kernel_grad *g, double *vals, int nvals, int64_t *count);
int slq_kernel_grad_reset(slq_kernel_grad *g);
int slq_kernel_grad_destroy(slq_kernel_grad *g);
/* The schedule of one update for n points, m columns and a chip of num_cus compute units (csrc/slq_kernelgrad.hpp:
 * kernel_grad_schedule): rows per block, row blocks, columns per chunk, chunks (launches), j slabs, then slab_begin[0 .. slabs]
 * (-1 beyond); nout >= 22. No HIP call. */
int slq_debug_kernel_grad_schedule(int64_t n, int m, int num_cus, int64_t *out, int nout);

/* ---- Cross-covariance products of the kernel operator -------------------------------------------------------
 * What a Gaussian-process posterior needs beside A^-1: the rectangular kernel matrix between NEW points and the operator's own.
 * For a kernel operator op (slq_kernel_create: points x_1..x_n, the centre mean(x) fixed at its creation, lengthscales l,
 * outputscale s, dtype F) and m new points x*_1..x*_m in the same d dimensions:
 *   z*_i  = (F)(((double)x*_i - mean(x)) / l)     the TRAINING centre, never the new points' own; double arithmetic rounded once, so
 *                                                 that a host model reproduces z* bit for bit
 *   r2_ij = max(0, fma(-2, z*_i.z_j, |z*_i|^2 + |z_j|^2))     NO diagonal rule: a new point equal to a training point gets the
 *                                                 r2 its arithmetic gives (0 up to rounding), not an exact 0
 *   C     = s phi(r2)                             m x n, NO noise term
 * The forward product is Y = C W (W n x b, Y m x b), the adjoint Y = C^T U (U m x b, Y n x b): one kernel with the two point sets
 * exchanging roles. C is never held. The summed points are walked in a fixed order, slab partials are summed in slab order and
 * nothing is atomic: identical calls give identical bits.
 * slq_kernel_cross_create: op must be a kernel operator of ctx; the object takes op's dtype (points: m x d words of it, row-major
 *   with leading dimension ldp >= d, on the host; _create_device: on the context's GPU, read back once for the check). It holds
 *   the raw new points, z*^T, |z*|^2 and its slab scratch (sized on first use, grown on demand). It reads op at every product and
 *   does not own it: destroy the cross object first. SLQ_EINVAL: a NULL handle, an operator of another kind or context, m < 1,
 *   ldp < d, a point that is not finite (the first one is named).
 * Hyperparameters: slq_kernel_set_parameters counts its calls on the operator; a cross object remembers the count its z* were
 *   derived at and re-derives them on the stream - no allocation, no upload - before its next product when the count has moved.
 *   It never writes the operator's z, |z|^2 or {s, sigma2}.
 * slq_kernel_cross_matmat: host panels in the object's dtype, column-major; trans == 0: X n x b (ldx >= n), Y m x b (ldy >= m);
 *   trans == 1: X m x b, Y n x b. Any b >= 1. Synchronises, like slq_operator_matmat.
 * slq_kernel_cross_dmat: the same on columns [i0, i0 + b) of IN and [o0, o0 + b) of OUT, asynchronous on the context stream;
 *   fp64 only (an fp32 object is refused, naming the dtype). IN must have n (trans == 0) or m (trans == 1) rows, OUT m or n.
 * Both: SLQ_EINVAL, nothing launched: a NULL handle, trans not 0 or 1, b < 1, a leading dimension or a row count that does not
 *   fit the direction, a column range outside its matrix, overlapping ranges of one matrix, a matrix of another context.
 * slq_debug_kernel_cross_points: z*^T (dpad x mpad; dpad = d rounded up to 4, mpad = m rounded up to 16) and |z*|^2 (mpad) from
 *   the device, in the object's dtype, after the re-derivation a product would do (either may be NULL). Synchronises.
 * A diagonal scale of the operator (slq_kernel_set_diag_scale) is IGNORED, as the noise is: C is defined on K0's points and profile. A
 *   product over the training points of a scaled operator carries the bits of the same product on the unscaled one. */
typedef struct slq_kernel_cross slq_kernel_cross;
int slq_kernel_cross_create(slq_context *ctx, slq_operator *op, int64_t m, const void *points, int64_t ldp, slq_kernel_cross **out);
int slq_kernel_cross_create_device(slq_context *ctx, slq_operator *op, int64_t m, const void *d_points, int64_t ldp, slq_kernel_cross **out);
int slq_kernel_cross_matmat(slq_kernel_cross *cross, int trans, const void *X, int64_t ldx, void *Y, int64_t ldy, int b);
int slq_kernel_cross_dmat(slq_kernel_cross *cross, int trans, slq_dmat *IN, int i0, slq_dmat *OUT, int o0, int b);
int slq_kernel_cross_destroy(slq_kernel_cross *cross);
int slq_debug_kernel_cross_points(slq_kernel_cross *cross, void *zt, void *nrm);
/* The schedule of one product with nrows output rows, nsum summed points and b columns on a chip of num_cus compute units
 * (csrc/slq_kernelcross.hpp: kernel_cross_schedule): rows per block, row blocks, 16-column tiles per workgroup, 256-column chunks,
 * slabs of the summed points (at most 64), tiles of 16 points per slab, then slab_begin[0 .. slabs] (-1 beyond); nout >= 71.
 * Slab z is the tiles [z * tiles_per_slab, (z + 1) * tiles_per_slab) cut at the end: what the kernel computes from its block
 * index. No HIP call. */
int slq_debug_kernel_cross_schedule(int64_t nrows, int64_t nsum, int64_t b, int num_cus, int64_t *out, int nout);

/* ---- Random Fourier features of the kernel operator (csrc/slq_kernelfeature.hpp) --------------------------------
 * The prior term of a pathwise posterior sample (gp.sample_paths). For a kernel operator op (scaled points z, outputscale s, dtype
 * F) and F2 >= 1 frequencies Omega (F2 x d, already rounded to F: the map is DEFINED on the rounded Omega)
 *   g_ij   = sum_k Omega_jk z_ik                                  row point i, frequency j
 *   Phi(z_i) = a [cos g_i1 .. cos g_iF2 | sin g_i1 .. sin g_iF2],   a = sqrt(s / F2), evaluated in F from s on the device
 *   Y = Phi W:  Y_ic = a sum_j (cos g_ij W[j, c] + sin g_ij W[F2 + j, c]),   W 2 F2 x b, column-major
 * Paired features, no random phase: Phi(z) Phi(z')^T = (s / F2) sum_j cos(omega_j.(z - z')) is exactly stationary. The profile is
 * the law Omega was drawn from (normal for rbf, Student-t with 2 nu degrees of freedom for the Matern family): the kernel has no
 * profile parameter. The row points are the operator's own (cross == NULL) or the new points z* of a slq_kernel_cross of the SAME
 * operator (training centre; re-derived on the stream first when the hyperparameters have moved, as before a cross product). No
 * noise term. sin and cos are the device library's accurate functions with full range reduction. Phi is never held; the
 * frequencies are walked in a fixed order, slab partials are summed in slab order and nothing is atomic: identical calls give
 * identical bits. s is read from device memory at every product: slq_kernel_set_parameters on op is honoured by the next one (the
 * lengthscales through z, the outputscale through a).
 * slq_kernel_feature_create: omega on the host, F2 x d words of op's dtype, row-major with leading dimension ld >= d. The object
 *   holds Omega^T (k-major, dpad x F2pad; dpad = d rounded up to 4, F2pad = F2 rounded up to 16; zeros in the padding) and its slab
 *   scratch. It reads op - and the cross object, if given - at every product and owns neither: destroy the feature map first.
 *   SLQ_EINVAL, nothing allocated: a NULL handle, an operator of another kind (a preconditioned operator is named: pass its base)
 *   or context, F2 < 1 or > 2^30, ld < d, a frequency that is not finite (the first one is named).
 * slq_kernel_feature_matmat: host panels in the object's dtype, column-major; W 2 F2 x b (ldw >= 2 F2), Y n x b - or m x b with a
 *   cross object - (ldy >= its rows). Any b >= 1. Synchronises.
 * slq_kernel_feature_dmat: the same on columns [i0, i0 + b) of IN (2 F2 rows) and [o0, o0 + b) of OUT (n or m rows), asynchronous
 *   on the context stream; fp64 only (an fp32 object is refused, naming the dtype). The two entries give the same bits.
 * Both: SLQ_EINVAL, nothing launched: a NULL handle, a cross object of another operator, b < 1, a leading dimension or a row
 *   count that does not fit, a column range outside its matrix, overlapping ranges of one matrix, a matrix of another context.
 * fp64 workgroups take at most 128 columns (two staged halves of W beside the accumulators), fp32 ones 256.
 * slq_debug_kernel_feature_frequencies: Omega^T as the device holds it, dpad x F2pad words of the object's dtype. Synchronises.
 * slq_debug_kernel_feature_schedule: the schedule of one product (csrc/slq_kernelfeature.hpp: kernel_feature_schedule) in the
 *   order of slq_debug_kernel_cross_schedule, the column chunks 128 wide with is_f64 != 0 and 256 otherwise; nout >= 71. No HIP call.
 * A diagonal scale of the operator (slq_kernel_set_diag_scale) is IGNORED, as the noise is: the features are those of K0's profile. */
typedef struct slq_kernel_feature slq_kernel_feature;
int slq_kernel_feature_create(slq_context *ctx, slq_operator *op, int64_t F2, const void *omega, int64_t ld, slq_kernel_feature **out);
int slq_kernel_feature_matmat(slq_kernel_feature *feat, slq_kernel_cross *cross, const void *W, int64_t ldw, void *Y, int64_t ldy, int b);
int slq_kernel_feature_dmat(slq_kernel_feature *feat, slq_kernel_cross *cross, slq_dmat *IN, int i0, slq_dmat *OUT, int o0, int b);
int slq_kernel_feature_destroy(slq_kernel_feature *feat);
int slq_debug_kernel_feature_frequencies(slq_kernel_feature *feat, void *omega_t);
int slq_debug_kernel_feature_schedule(int64_t nrows, int64_t F2, int64_t b, int num_cus, int is_f64, int64_t *out, int nout);
/* The adjoint of the map (csrc/slq_kernelfeatureadj.hpp): Z = Phi^T U,
 *   Z[j, c] = a sum_i cos g_ij U[i, c],     Z[F2 + j, c] = a sum_i sin g_ij U[i, c]
 * for U of n rows (or m, with a cross object of the same operator) and Z of 2 F2 rows in the row order of the forward product's W.
 * slq_kernel_feature_rmatmat: host panels in the object's dtype, column-major; U rows x b (ldu >= rows), Z 2 F2 x b (ldz >= 2 F2).
 *   Synchronises.
 * slq_kernel_feature_rdmat: the same on columns [i0, i0 + b) of IN (n or m rows) and [o0, o0 + b) of OUT (2 F2 rows), asynchronous
 *   on the context's stream; fp64 objects only. The same bits as the host entry.
 * Deterministic; s is read from the operator at every product. Refusals (SLQ_EINVAL, nothing launched) mirror the forward entries.
 * slq_debug_kernel_feature_adjoint_schedule: the schedule of one adjoint product (kernel_feature_adjoint_schedule: row blocks of
 *   the frequencies, slabs of the row points) in the out-array convention of slq_debug_kernel_feature_schedule. No device. */
int slq_kernel_feature_rmatmat(slq_kernel_feature *feat, slq_kernel_cross *cross, const void *U, int64_t ldu, void *Z, int64_t ldz, int b);
int slq_kernel_feature_rdmat(slq_kernel_feature *feat, slq_kernel_cross *cross, slq_dmat *IN, int i0, slq_dmat *OUT, int o0, int b);
int slq_debug_kernel_feature_adjoint_schedule(int64_t F2, int64_t nrows, int64_t b, int num_cus, int is_f64, int64_t *out, int nout);

/* ---- pivoted-Cholesky preconditioner of a kernel operator (csrc/slq_kernelprecond.hpp), fp64 only ----
 * K0 = s phi(r2) is the kernel matrix without noise, A = K0 + sigma2 I (sigma2 > 0). L (n x r, r <= rank_max <= 256) is the
 * greedy partial pivoted Cholesky factor of K0: the residual diagonal starts as d = s; step k takes p = argmax d (ties: the
 * smallest index), L[:, k] = (K0[:, p] - L[:, :k] L[p, :k]^T) / sqrt(d_p) with r2_pp = 0 exactly, d <- max(0, d - L[:, k]^2),
 * d_p <- 0 exactly; rows whose d_i is already 0 get L[i, k] = 0; it stops early when d_p <= max(tol, 64 eps) s, the remaining
 * columns stay zero and rank = the columns produced. P = L L^T + sigma2 I, and with L^T L = V diag(t) V^T
 *   P^{-1/2} = M = sigma^-1 (I - L G L^T),  G = V diag(g(t)) V^T,  g(t) = (1 - (1 + t / sigma2)^{-1/2}) / t,
 *   logdet P = sum log1p(t_i / sigma2) + n log sigma2.
 * The operator handed out is B = M A M, symmetric positive definite: logdet A = tr log B + logdet P, A^-1 y = M B^-1 M y, for
 * any L. All rank_max steps are launched back to back on the context stream; the pivot search is a two-level reduction across
 * kernel boundaries (no atomics), so identical calls give identical bits.
 * slq_kernel_precond_create: kernel_op must be a kernel operator of ctx in fp64 with sigma2 > 0; 1 <= rank_max <= 256 (clamped
 *   to n); tol >= 0. *out is an ordinary operator of kind "kernel_precond" whose product is B X: it works in
 *   slq_operator_matmat and in every plan, and goes with slq_operator_destroy. It reads kernel_op at every product and does not
 *   own it: destroy it first. L (n x rpad, row-major, rpad = rank_max rounded up to 16, zeros in unused columns), G and the
 *   scalars sit at device addresses that never change.
 * Staleness: after slq_kernel_set_parameters on kernel_op every product, apply and plan run on the preconditioned operator
 *   returns SLQ_EINVAL ("stale: call slq_kernel_precond_refresh") until slq_kernel_precond_refresh has refactored in place
 *   (same rank_max, same addresses: a captured graph sees the new factor).
 * slq_kernel_set_parameters, slq_kernel_cross_create, slq_kernel_grad_create and slq_operator_set_parameter refuse the
 *   preconditioned operator (SLQ_EINVAL).
 * slq_kernel_precond_info: rank_max, the rank reached, logdet P, the residual trace sum d, the largest t (any may be NULL).
 * slq_kernel_precond_get: pivots (rank_max, -1 beyond the rank), L (n x rank_max, column-major, ldl >= n), G (rank_max x
 *   rank_max, row-major), the eigenvalues t (rank_max) - any may be NULL. Synchronises.
 * slq_kernel_precond_apply: Y = P^{-1/2} X on host panels (column-major, ldx, ldy >= n; b >= 1). Synchronises.
 * slq_kernel_precond_apply_dmat: the same on columns [i0, i0 + b) of IN and [o0, o0 + b) of OUT (overlapping ranges of one
 *   matrix are refused), asynchronous on the context stream. The two entries give the
 *   same bits.
 * slq_debug_kernel_precond_addresses: the device addresses of L, G, the pivots and the residual diagonal as integers (tests).
 * The factor as operands of the gradient kernel. H = (L^T L + sigma2 I)^-1 = V diag(1 / (t + sigma2)) V^T is
 *   kept next to G (rpad x rpad, same upload, same staleness), so that P^-1 = (I - L H L^T) / sigma2.
 * slq_kernel_precond_columns: columns [o0, o0 + nc) of OUT = columns [c0, c0 + nc) of L (which = 0: a copy, bit for bit) or of
 *   L H (which = 1: on the matrix cores), 1 <= nc <= 64, 0 <= c0, c0 + nc <= rpad; asynchronous on the context stream, one writer
 *   per word: identical calls give identical bits. SLQ_EINVAL names the cause: not a preconditioned operator, stale, the column
 *   range, a row mismatch (OUT has other than n rows), another context.
 * slq_kernel_precond_trace_grad: vals = beta vals + alpha tr(P^-1 dA/dtheta) in the accumulator `grad`, which must have been created
 *   on the BASE operator of `pre` (SLQ_EINVAL "another operator" otherwise): sigma^-2 [tr D - sum_c (L H)_c^T D L_c] with tr D = 0
 *   for a lengthscale and n for the outputscale and the noise. The columns of the rank reached go through slq_kernel_grad_update 64
 *   at a time from two n x 64 matrices the preconditioner owns (allocated at the first call); one one-thread kernel then adds
 *   alpha n / sigma2 on the stream. Deterministic, asynchronous; the accumulator's column count is unchanged.
 * Not built for a base with a diagonal scale (slq_kernel_set_diag_scale): create and refresh refuse it, and so does every product,
 *   apply and plan run on a preconditioned operator whose base was scaled later (SLQ_EINVAL; clear the scale, then refresh). */
int slq_kernel_precond_create(slq_context *ctx, slq_operator *kernel_op, int rank_max, double tol, slq_operator **out);
int slq_kernel_precond_refresh(slq_operator *pre);
int slq_kernel_precond_info(const slq_operator *pre, int *rank_max, int *rank, double *logdet_p, double *residual_trace, double *t_max);
int slq_kernel_precond_get(slq_operator *pre, int32_t *pivots, double *L, int64_t ldl, double *G, double *eig);
int slq_kernel_precond_apply(slq_operator *pre, const void *X, int64_t ldx, void *Y, int64_t ldy, int b);
int slq_kernel_precond_apply_dmat(slq_operator *pre, slq_dmat *IN, int i0, slq_dmat *OUT, int o0, int b);
int slq_debug_kernel_precond_addresses(const slq_operator *pre, uint64_t *out4);
/* H as the device holds it: rank_max x rank_max, row-major (tests). Synchronises. */
int slq_debug_kernel_precond_h(slq_operator *pre, double *H);
int slq_kernel_precond_columns(slq_operator *pre, int which, int c0, int nc, slq_dmat *OUT, int o0);
int slq_kernel_precond_trace_grad(slq_operator *pre, slq_kernel_grad *grad, double alpha, double beta);
/* wall time of the last factorisation (create or refresh) in ms: out2[0] the launches up to the one synchronisation - the
 * rank_max steps and the Gram matrix -, out2[1] the host part: Jacobi, G and its upload (scripts/bench_kernelprecond.py). */
int slq_debug_kernel_precond_timing(const slq_operator *pre, double *out2);

/* ---- Gradients of the kernel operator with respect to the points (csrc/slq_kernelpointgrad.hpp), fp64 only ----
 * Notation as for the hyperparameter gradients: z the operator's rounded scaled points, chi = -2 dphi/dr2 (matern12: 0 where
 * r2 = 0), r2 the operator's own value - its operands, its order, its clamp and, on the training set, its diagonal rule.
 * Training form (slq_kernel_pointgrad_create): for columns of two device matrices Z, W (n rows), C = Z W^T, one update adds the n x d
 *   P[a][k] = sum_c Z_c^T (dA/dx_ak) W_c = -(s / l_k) sum_j (C_aj + C_ja) chi(r2_aj) (z_ak - z_jk).
 * Cross form (slq_kernel_pointgrad_create_cross): for the m new points z* of a slq_kernel_cross (training centre, no diagonal rule),
 *   U with m rows and W with n rows, the m x d
 *   R[a][k] = -(s / l_k) sum_j (sum_c U_ac W_jc) chi(r2(z*_a, z_j)) (z*_ak - z_jk),
 *   the gradient of sum_c U_c^T K(X*, X) W_c in the new points. P = R(Z, W) + R(W, Z) with both sets the training points: ONE
 *   one-sided kernel, run twice per 64-column chunk in that order (once, with twice the weight, where Z and W are the same matrix and
 *   column range). Centring drops out of a difference, so d/dx = (1 / l) d/dz exactly as written; the gradient is DEFINED as this
 *   smooth formula at the rounded z. The coordinate term is taken as the difference z_ak - z_jk: coincident points contribute
 *   exactly 0. Neither A nor C nor a derivative tile is held; nothing is atomic and the slab partials are added in slab order:
 *   identical calls give identical bits.
 * slq_kernel_pointgrad_create: op must be a kernel operator in fp64 of ctx (SLQ_EINVAL names the kind - a preconditioned operator
 *   is "kernel_precond": pass its base - or the dtype). The accumulator reads op at every update and does not own it: destroy the
 *   accumulator first. The values start at 0.
 * slq_kernel_pointgrad_create_cross: borrows the cross object AND its operator (destroy the accumulator first); an fp32 cross
 *   object is refused. After slq_kernel_set_parameters the z* are re-derived on the stream before the next update, as before a
 *   cross product.
 * slq_kernel_pointgrad_update: vals = beta * vals + alpha * (P or R over columns [c0, c0 + m) of Z_or_U and [w0, w0 + m) of W);
 *   count += m. Columns go 64 to a launch; wider ranges fold in one after the other. Asynchronous on the context stream. beta == 0
 *   does not read the old values. The operator's parameters are read as they are at the call (the contract of
 *   slq_kernel_grad_update). SLQ_EINVAL, nothing launched and the values untouched: a NULL handle, a column range outside its
 *   matrix, m < 1, a row count that does not fit the form (Z_or_U: n, or m new points; W: n), an object of another context, a
 *   non-finite alpha or beta.
 * slq_kernel_pointgrad_get: rows x d values, row-major like the points with leading dimension ld >= d, and the columns folded in so
 *   far (either may be NULL). Synchronises.
 * slq_kernel_pointgrad_reset: values and count back to 0 (asynchronous).
 * slq_kernel_precond_trace_pointgrad: vals = beta vals + alpha tr(P^-1 dA/dx) = beta vals - alpha sigma^-2 sum_c (L H)_c^T (dA/dx) L_c
 *   (tr dA/dx = 0), the columns of the rank reached 64 at a time through the matrices slq_kernel_precond_trace_grad uses. `grad`
 *   must be a training-form accumulator on the BASE of `pre`; a stale preconditioner is refused. The column count is unchanged.
 * A diagonal scale of the operator (slq_kernel_set_diag_scale): the training form is not built for it (create and every update refuse
 *   with SLQ_EINVAL); the cross form is defined on K0's points and profile and ignores it, as a cross product does. */
typedef struct slq_kernel_pointgrad slq_kernel_pointgrad;
int slq_kernel_pointgrad_create(slq_context *ctx, slq_operator *op, slq_kernel_pointgrad **out);
int slq_kernel_pointgrad_create_cross(slq_context *ctx, slq_kernel_cross *cross, slq_kernel_pointgrad **out);
int slq_kernel_pointgrad_update(slq_kernel_pointgrad *g, slq_dmat *Z_or_U, int c0, slq_dmat *W, int w0, int m, double alpha, double beta);
int slq_kernel_pointgrad_get(slq_kernel_pointgrad *g, double *vals, int64_t ld, int64_t *count);
int slq_kernel_pointgrad_reset(slq_kernel_pointgrad *g);
int slq_kernel_pointgrad_destroy(slq_kernel_pointgrad *g);
int slq_kernel_precond_trace_pointgrad(slq_operator *pre, slq_kernel_pointgrad *grad, double alpha, double beta);
/* The schedule of one pass with nrows row points and nsum summed points on a chip of num_cus compute units
 * (csrc/slq_kernelpointgrad.hpp: kernel_pointgrad_schedule): rows per block, row blocks, factor columns per launch, slabs of the
 * summed points (at most 64), tiles of 16 points per slab, then slab_begin[0 .. slabs] (-1 beyond); nout >= 70. No HIP call. */
int slq_debug_kernel_pointgrad_schedule(int64_t nrows, int64_t nsum, int num_cus, int64_t *out, int nout);

/* Per-kernel device time accumulated by HIP events on the context stream (for bench.py's
 * roofline line). enable != 0 turns event recording on for subsequent slq_plan_run calls. */
enum {
  SLQ_K_SPMM = 0,    /* sweep A: panel SpMM + three-term update + alpha partials                  */
  SLQ_K_AXPY_NORM,   /* sweep B (orth = 0): w -= alpha q_c, ||w||^2 partials                       */
  SLQ_K_REORTH_DOT,  /* sweep B (orth > 0): w -= alpha q_c, c = Q_r^T w partials                   */
  SLQ_K_REORTH_UPD,  /* sweep C: w -= Q_r c, ||w||^2 partials                                      */
  SLQ_K_FINALIZE,    /* all per-step scalar kernels (partials -> alpha/beta/coefficients)           */
  SLQ_K_PROBES,      /* probe generation / layout                                                   */
  SLQ_K_QUADRATURE,  /* tridiagonal eigensolve + f reduction                                        */
  SLQ_K_COMBINE,     /* f(A)x = sum_t g_t W_t over the kept basis (slq_plan_fun_action; not a recurrence sweep), and the
                        accumulation launches of a recompute plan's replay and of a Chebyshev action (their passes count in
                        their usual classes) */
  SLQ_K_COUNT
};
typedef struct {
  double ms[SLQ_K_COUNT];       /* summed device time per class                                   */
  int64_t launches[SLQ_K_COUNT];
} slq_profile;
int slq_plan_profile_enable(slq_plan *plan, int enable);
/* Byte accounting of the deep-window update sweep (orth > 8), which reads a ring column only when some probe of the panel has a non-zero projection on it - the
 * reference skips a projection per probe below its threshold, src/primate/include/lanczos.h:62 -: columns read / columns offered, summed over launches and panels
 * since the last reset. Synchronises. */
int slq_plan_sweep_columns(slq_plan *plan, uint64_t *read, uint64_t *offered, int reset);
/* The oldest column of a full three-column window (ring-fed Gram sequence, orth = 3) is read by the update pass only where its zero projection is not
 * certified from the inner products the step already has (SLQ_OMEGA: 1 on, 0 every column read, 2 verify: every column read and the certificate checked
 * against the measurement). out: columns offered, columns read, rescues (the missing entry measured by a dot of its own), verify-mode violations,
 * read -> skip transitions; summed over steps and panels since the last reset; zeros for a plan that offers nothing. Synchronises.
 * The last step of a run is counted by the run's closing tail (slq_plan_closing_state): this call, _verify, _census, _flags and slq_plan_get_tridiag launch a
 * pending one, but new probes drop it, so a run whose tail nobody asked for before the next probes adds its steps 2 .. deg - 2 only (`panels` offered fewer,
 * and whatever that step read or rescued). Read or reset the counters after each run, or create the plan under SLQ_LAST_STORE=2, for sums over every step. */
int slq_plan_window_columns(slq_plan *plan, int64_t out[5], int reset);
/* Which kernel computes the product of a plan on a dense operator, and over how many K slabs (a diagnostic entry: what the plan will launch, from the
 * panel width, the operator's leading dimension and the SLQ_DENSE_* switches read when it was created). kernel: 0 the operator is not dense,
 * 1 k_dense_panel, 2 k_dense_mfma_3term, 3 k_dense_mfma_tile, 4 k_dense_mfma_lds, 5 k_dense_mfma32_lds; ksplit: workgroups (slabs) the K range is
 * split over, 0 for the kernels without slabs. A plan on a kernel operator (slq_kernel_create) answers kernel 0 and, in ksplit, the j slabs of its
 * product (0: one slab, written straight into the product panel). kernel or ksplit may be NULL. */
int slq_plan_dense_path(slq_plan *plan, int *kernel, int *ksplit);
/* ... the plan's mode (0 where nothing is offered) and, from verify runs since the last reset of those counters: out[0] the largest one-step innovation
 * |measured - predicted| in units of eps ||A||_inf, out[1] the smallest (tol - |measured|) / rho (inf: none seen), out[2], out[3] the constants c and kappa
 * of the certificate, out[4] ||A||_inf. mode or out may be NULL. */
int slq_plan_window_verify(slq_plan *plan, int *mode, double out[5]);
/* Census of the last run of a ring-fed Gram plan created under SLQ_OMEGA=2: out[(j * 9 + i) * panels + panel] = probes of the panel with a non-zero
 * projection coefficient at window position i of step j; len must be (deg + 1) * 9 * panels. */
int slq_plan_window_census(slq_plan *plan, int32_t *out, int64_t len);
/* The per-step flags of the last run: read[j * panels + panel] = 1 where the panel's update pass of step j read the oldest column, rescue[...] = 1 where its
 * entry was measured by the rescue kernel; len must be (deg + 1) * panels. (slq_plan_window_verify, _census and _flags are diagnostic entries: the tests' and
 * the verify mode's view of the recurrence, not part of what a driver needs.) */
int slq_plan_window_flags(slq_plan *plan, int32_t *read, int32_t *rescue, int64_t len);
int slq_plan_profile_read(slq_plan *plan, slq_profile *out, int reset);

/* Failure reporting of the ring-fed tile pass (k_csr_ring_pass). Every wait inside that kernel is bounded; a workgroup
 * whose wait runs out raises a device word and leaves, and every accessor that hands results of a run to the host
 * (slq_plan_get_tridiag, _quadrature, _get_basis, _fun_action[_dmat], slq_diag_update, the one-shot entries) then returns
 * SLQ_EHIP instead of undefined numbers (the reference's kernel has no failure mode of its own:
 * src/primate/include/lanczos.h:92-149 is noexcept host code). Two hooks for the tests:
 *   slq_debug_ring_flag_status   the flag -> status translation those accessors share (no device work: CPU-testable)
 *   slq_debug_plan_poke_ring_flag  sets a plan's device word as an aborting workgroup would */
int slq_debug_ring_flag_status(int flag);
int slq_debug_plan_poke_ring_flag(slq_plan *plan, int value);
/* test hook: mark a plan as holding nstale stale ring columns (what the drop-in entry does to its own plan) */
int slq_debug_plan_mark_stale(slq_plan *plan, int nstale);
/* What step j of a run launches, as the library decides it, without a device (csrc/slq_sequence.hpp: step_shape). facts: the
 * 27 facts of a plan and its operator in the order of seq::facts_from_array (facts[2]: the operator's tiles, 0 none / 1 landed
 * behind barriers / 2 ring-fed); out: the 18 values of seq::shape_to_array, then what slq_plan_describe reports as
 * `sequence` for such a plan. No HIP call. */
int slq_debug_step_shape(const int *facts, int nfacts, int j, int prev_xt, int *out, int nout);
/* Whether a plan of these facts leaves its closing tail to the first request (seq::has_lazy_tail; lazy_close: 0 for a plan created under
 * SLQ_LAST_STORE=2, which keeps the pass in the run, else 1; values_fixed: 0 for an affine operator A + t B, whose values
 * slq_operator_set_parameter rewrites under a live plan - its plans have no lazy tail -, else 1): *out = 1 or 0. No HIP call. */
int slq_debug_lazy_tail(const int *facts, int nfacts, int lazy_close, int values_fixed, int *out);
/* The same for step j of a Chebyshev run of facts[7] (deg) steps (seq::cheb_step_shape, derived from step_shape's answer at
 * orth = 0): out receives the 9 values of seq::cheb_shape_to_array - sweeps, tiled, gen, pipe_on, the update pass's xt word,
 * the sweeps' product kernel and its grid, the grid behind the partials, alpha_pass (always 0). No HIP call. */
int slq_debug_cheb_step_shape(const int *facts, int nfacts, int j, int *out, int nout);
/* The accumulation launches of an action of nsteps steps (csrc/slq_sequence.hpp: cheb_action_schedule), in launch order: piece
 * i consumes the ring columns t0[i] .. t0[i] + nc[i] - 1 (t0, nc: the first cap pieces are written; either may be NULL);
 * *npieces their number, *ring_slots the ring of such a plan, *acc_cols the columns a launch consumes at most. No HIP call. */
int slq_debug_cheb_action_schedule(int nsteps, int *t0, int *nc, int cap, int *npieces, int *ring_slots, int *acc_cols);
/* The layout a CSR operator over this pattern would be created with, as the library decides it, without a device
 * (csrc/slq_layout.hpp: layout_prefilter + decide_layout; the operator switches are read from the environment as a creation
 * reads them). plain != 0: the affine operator's kind (caller's order, no tiles). perm_out [n]: stored row i = caller row
 * perm_out[i], written only for a reordered operator; tile_row_out [ntiles + 1 <= ntile_cap]: first stored row of every tile,
 * written only with tiles; xcd_tile_out [9]: the tile range of every XCD chunk; info_out [4]: have_tiles, ntiles, reordered,
 * rms in-chunk |i - j| of the stored nonzeros. No HIP call. */
int slq_debug_csr_layout(int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colind, int plain, int32_t *perm_out,
                         int32_t *tile_row_out, int64_t ntile_cap, int32_t *xcd_tile_out, double *info_out);
/* What creating a plan decides (csrc/slq_plan_shape.hpp: plan_shape), without a device: the facts of operator, context and
 * request as an array in the order of plan_facts_to_array (kNumPlanFacts values), the shape - geometry, grids, tile stream,
 * sequence flags, the table of the plan's device allocations {id, bytes, zeroed, counted} and the offsets inside its two
 * carved blocks - in the order of plan_shape_to_array (kNumPlanShape values). The plan switches are read from the environment
 * as a creation reads them. No HIP call. slq_debug_plan_shape_of returns the facts and the shape a live plan was created from. */
int slq_debug_plan_shape(const double *facts, int nfacts, double *out, int nout);
int slq_debug_plan_shape_of(const slq_plan *plan, double *facts_out, int nfacts, double *shape_out, int nout);

/* ---- one-shot entries ---------------------------------------------------------------------------- */
/* P probes in one call: the batched counterpart of the Python loop at
 * src/primate/operators.py:145-150. X: host column-major n x nprobes, or NULL to draw probes on
 * the device (pdf, seed, probe_offset). quad_out: nprobes doubles. nodes_out / weights_out:
 * nprobes x deg row-major doubles or NULL. */
int slq_quad_batch(slq_context *ctx, slq_operator *op, const void *X, int64_t ldx, int pdf,
                   uint64_t seed, uint64_t probe_offset, int nprobes, int deg, double rtol,
                   int orth, int fun_id, const double *fun_params, double *quad_out,
                   double *nodes_out, double *weights_out);

/* Y[:, i] = f(A) X[:, i] for nvec columns in one call: the batched counterpart of
 * MatrixFunction._matvec (src/primate/operators.py:102-124: Lanczos with the full basis kept,
 * eigh_tridiagonal, Q (Y (f(theta) * Y[0,:])) ||x||). X, Y: host column-major, operator dtype. Built-in
 * fun ids only. Columns are processed in as few lock-step batches as the free device memory allows. */
int slq_fAv_batch(slq_context *ctx, slq_operator *op, const void *X, int64_t ldx, int nvec, int deg,
                  double rtol, int orth, int fun_id, const double *fun_params, void *Y, int64_t ldy);
/* The same with the plan kind chosen: basis_mode 1 kept basis (what slq_fAv_batch does), 2 recompute plans (two passes per
 * batch, a footprint independent of deg), 0 automatic: the kept basis when a plan for ALL nvec columns fits the free device
 * memory (its bytes + 1 GiB <= free), otherwise recompute plans - for all columns when that fits, else halved batches.
 * basis_used (or NULL) receives the kind taken. */
int slq_fAv_batch_mode(slq_context *ctx, slq_operator *op, const void *X, int64_t ldx, int nvec, int deg, double rtol, int orth,
                       int fun_id, const double *fun_params, int basis_mode, void *Y, int64_t ldy, int *basis_used);

/* Single-vector drop-in for primate._lanczos.lanczos (src/primate/_lanczos.cpp:88-99), host
 * pointers, same in/out contract: v (n) is scratch and is clobbered; alpha, beta (deg+1) and
 * Q (n x ncv column-major) are written in place; beta[0] = 0. Q's incoming contents take part in
 * the re-orthogonalisation exactly as in the reference (columns other than ncv-1 and 0 are not
 * cleared, src/primate/include/lanczos.h:118-121). Returns the number of executed steps (>= 1)
 * or a negative error code. */
int slq_lanczos_f64(slq_context *ctx, slq_operator *op, double *v, int deg, double rtol, int orth,
                    double *alpha, double *beta, double *Q, size_t ncv);
int slq_lanczos_f32(slq_context *ctx, slq_operator *op, float *v, int deg, float rtol, int orth,
                    float *alpha, float *beta, float *Q, size_t ncv);

#ifdef __cplusplus
}
#endif
#endif /* SLQ_H */
