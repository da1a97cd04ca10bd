// slq_kernelpointgrad.hip — the instantiations of k_kernel_pointgrad (slq_kernelpointgrad.hpp) in a translation unit
// of their own, so that the build stays parallel: 4 profiles x 2 coordinate depths, and the sum kernel. The C-ABI over them
// (slq_kernel_pointgrad_*) is in slq.hip and calls the two launch functions below.
#include <hip/hip_runtime.h>

#define SLQ_KERNELPOINTGRAD_DEVICE 1
#include "slq_kernelpointgrad.hpp"

namespace slq {

bool kernel_pointgrad_launch(int profile, const KernelPointGradSchedule &S, const KernelPointGradArgs &a, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  const dim3 g(S.nrow_blocks, S.nslabs), b(64 * kKernelWaves);
  return kernel_for_profile(profile, [&](auto P) {
    return kernel_for_dq(a.dq, [&](auto DQ) {
      k_kernel_pointgrad<P(), DQ()><<<g, b, 0, st>>>(a.nrows, a.rpad, a.nsum, a.spad, a.dq, a.diagonal, a.rzt, a.rnrm, a.szt, a.snrm, a.U, a.W, a.mc,
                                                     S.tiles_per_slab, a.part);
      return true;
    });
  });
}

void kernel_pointgrad_sum_launch(int64_t nrows, int d, int dpad, int nslabs, const double *part, const double *params, const KernelPointGradScale &sc,
                                 double alpha, double beta, double *vals, void *stream) {
  const dim3 g((unsigned)((nrows * d + 255) / 256)), b(256);
  k_kernel_pointgrad_sum<<<g, b, 0, (hipStream_t)stream>>>(nrows, d, dpad, nslabs, part, params, sc, alpha, beta, vals);
}

}  // namespace slq
