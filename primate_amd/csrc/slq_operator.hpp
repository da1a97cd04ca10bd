// slq_operator.hpp — the operator handle of slq.hip and what it owns, as values: one owning device buffer (DevBuf), a stored CSR
// (CsrArrays), a ring-fed tile stream (TileStream), a set of scaled points (KernelPoints). Destroying an operator is `delete`: every device array is a member that frees
// itself, so an array added here cannot leak and a half-built operator goes with everything it has so far.
#pragma once
#include "../../include/slq.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

#include "slq_common.hpp"
#include "slq_kernelop.hpp"  // KernelScale, k_kernel_rescale
#include "slq_switches.hpp"

namespace slq {

// bytes the live DevBufs of the process hold (slq_debug_operator_device_bytes: tests)
inline std::atomic<int64_t> g_devbuf_bytes{0};

// A device allocation that frees itself: every device array an operator or a side object (accumulators, cross objects, feature maps,
// device matrices) owns, and the scratch of a build. Move-only.
struct DevBuf {
  void *p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p(o.p), nbytes(o.nbytes) { o.p = nullptr, o.nbytes = 0; }
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) {
      release();
      std::swap(p, o.p);
      std::swap(nbytes, o.nbytes);
    }
    return *this;
  }
  ~DevBuf() { release(); }
  void release() {
    if (p) {
      hipFree(p);
      g_devbuf_bytes -= (int64_t)nbytes;
    }
    p = nullptr, nbytes = 0;
  }
  hipError_t alloc(size_t bytes) {
    release();
    const hipError_t e = hipMalloc(&p, std::max<size_t>(bytes, 16));
    if (e != hipSuccess) p = nullptr;
    else nbytes = bytes, g_devbuf_bytes += (int64_t)bytes;
    return e;
  }
  size_t bytes() const { return nbytes; }  // as asked for (the allocation itself is never shorter than 16)
  explicit operator bool() const { return p != nullptr; }
  template <typename T> T *as() const { return (T *)p; }

 private:
  size_t nbytes = 0;
};

// A CSR on the device: rowptr [nrows + 1], colind and vals with kCsrPad spare entries behind the nnz stored ones - the batched row
// gather (slq_kernels.hpp: gather_row_uniform) loads indices and values 8 at a time and may read (never use) up to 7 entries past a
// row's end. Kernels receive the plain pointers, taken at the launch site.
struct CsrArrays {
  DevBuf rowptr, colind, vals;
  int64_t nnz = 0;
  // colind and vals alone, for a row pointer that is filled first (the device-side build counts, then fills); the pad is cleared on `st`
  hipError_t alloc_entries(int64_t nnz_, size_t es, hipStream_t st) {
    nnz = nnz_;
    hipError_t e = colind.alloc(((size_t)nnz + kCsrPad) * 4);
    if (e == hipSuccess) e = vals.alloc(((size_t)nnz + kCsrPad) * es);
    if (e == hipSuccess) e = hipMemsetAsync(colind.as<int32_t>() + nnz, 0, kCsrPad * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(vals.as<char>() + (size_t)nnz * es, 0, kCsrPad * es, st);
    return e;
  }
  hipError_t alloc(int64_t nrows, int64_t nnz_, size_t es, hipStream_t st) {
    const hipError_t e = rowptr.alloc((size_t)(nrows + 1) * 4);
    return e == hipSuccess ? alloc_entries(nnz_, es, st) : e;
  }
  void release() {
    rowptr.release(), colind.release(), vals.release();
    nnz = 0;
  }
  explicit operator bool() const { return (bool)rowptr; }
  const int32_t *rp() const { return rowptr.as<int32_t>(); }
  const int32_t *ci() const { return colind.as<int32_t>(); }
};

// What a ring-fed pass reads: 64 R descriptor words per tile, the tiles' CSR records, the tile ranges of the eight XCD chunks, the
// longest line list of a tile and whether every row's entries are padded to a multiple of four (build_ring_stream: pad_rows).
// max_lines may be known of a stream that was then not built (an upper-triangle stream that lands too many panel rows per row).
struct TileStream {
  DevBuf desc, rec;
  int32_t xcd_tile[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  int max_lines = 0;
  bool padded = false;
  explicit operator bool() const { return (bool)desc; }
};
// ... over the full rows, and over the upper triangle (exactly symmetric operators: the alpha-only pass) where the operator has it
struct TileStreamPair {
  TileStream full, upper;
  bool tried = false;  // merged streams: built, or found unbuildable, by the first plan that asked (ensure_ring_stream)
};

// A set of scaled points on the device (slq_kernelop.hpp): one allocation raw points (n x d, row-major) | z transposed (dpad x
// npad) | |z|^2 (npad) | two words {s, sigma2}, each on a 256-byte boundary. The addresses never change after alloc_and_upload - a
// captured graph reads them - and rescale() rewrites everything behind the raw points in place.
struct KernelPoints {
  DevBuf buf;
  void *zt = nullptr, *nrm = nullptr, *params = nullptr;
  int64_t n = 0, npad = 0;
  int d = 0, dpad = 0;
  // n_ points of d_ coordinates, ldp words apart, on the host or (on_device) on the device: checked finite on the host - of device
  // points a packed host copy is taken, once - and uploaded on `st`. bad->what != KERNEL_OK: the first coordinate that is not
  // finite, and nothing is allocated. mean (may be NULL): kernel_column_means of the points. The caller's host points are read
  // until `st` has run.
  hipError_t alloc_and_upload(int64_t n_, int d_, const void *points, int64_t ldp, bool on_device, int dtype, hipStream_t st, KernelBad *bad, double *mean = nullptr) {
    const size_t es = dtype == SLQ_F64 ? 8 : 4;
    std::vector<char> host;
    if (on_device) {
      host.resize((size_t)n_ * d_ * es);
      const hipError_t e = hipMemcpy2D(host.data(), (size_t)d_ * es, points, (size_t)ldp * es, (size_t)d_ * es, (size_t)n_, hipMemcpyDeviceToHost);
      if (e != hipSuccess) return e;
      points = host.data(), ldp = d_;
    }
    *bad = dtype == SLQ_F64 ? kernel_first_bad_point<double>(n_, d_, (const double *)points, ldp) : kernel_first_bad_point<float>(n_, d_, (const float *)points, ldp);
    if (bad->what != KERNEL_OK) return hipSuccess;
    if (mean && dtype == SLQ_F64) kernel_column_means<double>(n_, d_, (const double *)points, ldp, mean);
    else if (mean) kernel_column_means<float>(n_, d_, (const float *)points, ldp, mean);
    n = n_, npad = kernel_npad(n_), d = d_, dpad = kernel_dpad(d_);
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t b_raw = up((size_t)n * d * es), b_zt = up((size_t)dpad * (size_t)npad * es), b_nrm = up((size_t)npad * es);
    hipError_t e = buf.alloc(b_raw + b_zt + b_nrm + 256);
    if (e != hipSuccess) return e;
    zt = buf.as<char>() + b_raw;
    nrm = (char *)zt + b_zt;
    params = (char *)nrm + b_nrm;
    e = hipMemcpy2DAsync(buf.p, (size_t)d * es, points, (size_t)ldp * es, (size_t)d * es, (size_t)n, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && on_device) e = hipStreamSynchronize(st);  // (the host copy goes with this frame)
    return e;
  }
  // z, |z|^2, s and sigma2 from the raw points, on `st` (no allocation, no upload)
  hipError_t rescale(const KernelScale &sc, double s, double noise, int dtype, hipStream_t st) const {
    const dim3 g((unsigned)((npad + 255) / 256));
    if (dtype == SLQ_F64)
      k_kernel_rescale<double><<<g, dim3(256), 0, st>>>((int)n, (int)npad, d, dpad, buf.as<const double>(), sc, (double *)zt, (double *)nrm, (double *)params, s, noise);
    else
      k_kernel_rescale<float><<<g, dim3(256), 0, st>>>((int)n, (int)npad, d, dpad, buf.as<const float>(), sc, (float *)zt, (float *)nrm, (float *)params, s, noise);
    return hipGetLastError();
  }
  // what the kernels read, as it is on the device now, to host arrays (any may be NULL); the caller has waited for the stream
  hipError_t download(void *zt_h, void *nrm_h, void *params_h, int dtype) const {
    const size_t es = dtype == SLQ_F64 ? 8 : 4;
    hipError_t e = hipSuccess;
    if (zt_h) e = hipMemcpy(zt_h, zt, (size_t)dpad * (size_t)npad * es, hipMemcpyDeviceToHost);
    if (e == hipSuccess && nrm_h) e = hipMemcpy(nrm_h, nrm, (size_t)npad * es, hipMemcpyDeviceToHost);
    if (e == hipSuccess && params_h) e = hipMemcpy(params_h, params, 2 * es, hipMemcpyDeviceToHost);
    return e;
  }
};


// What a preconditioned kernel operator (OP_KERNEL_PRECOND, slq_kernelprecond.hpp) owns: the factor L (n x rpad, row-major, zeros
// in unused columns), G and H (rpad x rpad each), the residual diagonal and the device words of the factor's steps - all at addresses that
// never change after creation, so that a captured graph sees a refreshed factor - and the host record of the last factorisation.
struct KernelPrecond {
  slq_operator *base = nullptr;  // not owned: its points, profile and scalars are read at every product
  int rank_max = 0, rpad = 0, rank = 0;
  double tol = 0.0;
  uint64_t epoch = 0;  // the base's k_epoch the factor was built at
  DevBuf L, G, H, dres;  // H = (L^T L + sigma2 I)^-1: uploaded with G, stale when G is (§4.19)
  DevBuf words;        // pivots[rank_max] | rank | (pad to 8 bytes) | d_p per step [rank_max] | partials: 2 x nparts doubles, 2 x nparts ints
  int *pivots = nullptr, *rank_d = nullptr, *pi = nullptr;
  double *dpiv = nullptr, *pv = nullptr;
  DevBuf scratch, stage_in, stage_out;  // of the stand-alone applies (grown on demand); a plan has its own
  DevBuf cols;                          // two n x 64 column-major chunks, L H and L, of slq_kernel_precond_trace_grad (allocated at its first call)
  double logdet_p = 0.0, residual_trace = 0.0, t_max = 0.0;
  std::vector<double> eig;  // the eigenvalues of L^T L (rank_max of them)
  double device_ms = 0.0, host_ms = 0.0;  // wall time of the last factorisation: launches up to the synchronisation, then Jacobi, G and its upload
};

}  // namespace slq

struct slq_context;

struct slq_operator {
  slq_context *ctx = nullptr;
  int kind = 0, dtype = 0;
  int64_t n = 0, nnz = 0;
  slq::CsrArrays csr;      // the stored rows (OP_GRAM: A, mrows rows; OP_DENSE: vals alone, the matrix)
  int64_t lda = 0;
  slq_matvec_fn fn = nullptr;
  void *user = nullptr;
  slq_matmat_device_fn dev_fn = nullptr;  // OP_DEVICE_CALLBACK: Y = A X on device buffers, enqueued on our stream
  slq::DevBuf perm_d, inv_perm_d;  // device: stored row i = caller row perm[i], caller row r = stored row inv_perm[r] (empty: not reordered)
  std::vector<int32_t> perm_h;     // host copy (diag un-permutation); empty: not reordered
  // workgroup LDS tiles of the fused passes (tile_ptr empty: none; SLQ_TILES). tile_cols, lcol and self_idx are read by
  // k_csr_tile_pass only: ring-sized tiles carry them inside their records
  struct TileLists {
    slq::DevBuf tile_row, tile_ptr, tile_cols, lcol, self_idx;  // (slq_common.hpp: TileMeta)
    int32_t xcd_tile[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int max_cols = 0;
  } tiles;
  bool tiles_ringed = false;  // ... built to the caps of the ring-fed passes (SLQ_TILES=2), which read streams[]:
  // by log2 R (slq_plan_shape.hpp: STREAM_BASE, STREAM_MERGED2, STREAM_MERGED4) - [0] the tiles as clustered, whose upper stream has
  // tiles of its own, runs of the base tiles (regroup_upper_tiles, r04); [1], [2] R = 2, 4 consecutive tiles merged into one for
  // narrow panels (slq_ring.hpp), built the first time a plan asks for them (ensure_ring_stream), under merged_lock
  slq::TileStreamPair streams[3];
  mutable std::mutex merged_lock;  // (taken only where tiles_ringed holds)
  double upper_per_row = 0.0;      // distinct panel rows per row streams[0].upper lands (what decides whether the alpha-only pass takes it)
  // exactly symmetric CSR only: upper triangle (diagonal + 2x strict upper) for the alpha pass, whose
  // q^T A q = sum_i q_i (a_ii q_i + 2 sum_{j>i} a_ij q_j) then gathers half the panel rows (empty: none)
  slq::CsrArrays upper;
  double rms_dist = -1.0;    // rms |i - j| over the stored nonzeros inside an XCD chunk (-1: unknown)
  double far_per_row = 0.0;  // stored nonzeros per row with |i - j| > 4096 (0 when unknown: device-resident CSR)
  double norm_inf = -1.0;    // largest absolute row sum of a CSR operator (-1: not taken yet; operator_norm_inf takes it once, on the device)
  // OP_GRAM (x -> A^T (A x), A is mrows x n): csr holds A, transposed its transpose (n rows)
  int64_t mrows = 0;
  slq::CsrArrays transposed;
  slq::DevBuf dense_t;  // OP_DENSE, non-symmetric input only: the transpose, for the kernel that walks A by columns (empty: A == A^T)
  // affine CSR operator A + t B (slq_csr_affine_create): values of A and B on the union pattern (csr.vals = va + t vb)
  slq::DevBuf vals_a, vals_b;
  slq::OperatorSwitches sw;  // the switches as they were when the operator was created (slq_switches.hpp)
  // OP_KERNEL (slq_kernelop.hpp): the points, their z and |z|^2, s and sigma2 in two device words - all at addresses that never
  // change, so that a captured graph sees a hyperparameter change. nnz reports n d.
  int k_profile = 0;
  slq::KernelPoints k_pts;
  std::unique_ptr<slq::KernelScale> k_scale;  // host: the centre of the points and the lengthscales per dimension
  double k_s = 1.0, k_noise = 0.0;
  std::unique_ptr<slq::KernelPrecond> pre;  // OP_KERNEL_PRECOND: B = M A M on the points of pre->base
  uint64_t k_epoch = 0;  // host: incremented by every slq_kernel_set_parameters; a slq_kernel_cross compares it with the one its z* were derived at
  // the diagonal scale c of slq_kernel_set_diag_scale: A = s diag(c) phi(r2) diag(c) + sigma2 I. k_c: npad words in
  // the operator's dtype, allocated by the first set and never moved (a captured graph of the scaled product sees new values);
  // k_c_stage: the n doubles as given, on their way to k_kernel_diag_scale; k_c_host: c as rounded, for slq_kernel_get_diag_scale.
  // Setting or clearing the scale bumps k_epoch; whether it is set is part of a plan's graph key (scaled and unscaled are two kernels).
  bool k_scaled = false;
  slq::DevBuf k_c, k_c_stage;
  std::vector<double> k_c_host;
  // OP_TOEPLITZ (slq_toeplitz.hpp): the symbol in the order the forward passes leave (L complex words of the dtype, 1/L
  // folded in), the W_1024 table and the twiddles of the outer levels - at addresses that never change after creation, so that a captured
  // graph computes with the values of the last slq_toeplitz_set_values. tz_c, tz_r: the values as rounded (host). nnz reports 2n - 1.
  slq::DevBuf tz_sym, tz_tab, tz_tw[2];
  std::vector<double> tz_c, tz_r;
  bool tz_symmetric = true;
};
