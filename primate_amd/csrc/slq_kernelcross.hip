// slq_kernelcross.hip — the instantiations of k_kernel_cross (slq_kernelcross.hpp) in a translation unit of their
// own, so that the build stays parallel: 2 dtypes x 4 profiles x 5 column widths x 2 coordinate depths. The C-ABI over them
// (slq_kernel_cross_*) is in slq.hip and calls the two launch functions below.
#include <hip/hip_runtime.h>

#define SLQ_KERNELCROSS_DEVICE 1
#include "slq_kernelcross.hpp"

namespace slq {

bool kernel_cross_launch(int dtype_is_f64, int profile, const KernelSchedule &S, const KernelCrossArgs &a, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  return dtype_is_f64 ? kernel_cross_launch_profile<double>(profile, S, a, st) : kernel_cross_launch_profile<float>(profile, S, a, st);
}

void kernel_cross_sum_launch(int dtype_is_f64, int64_t nrows, int b, int nslabs, const void *part, int64_t slab_stride, void *Y, int64_t ldy, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  const dim3 g((unsigned)((nrows * b + 255) / 256)), blk(256);
  if (dtype_is_f64) k_kernel_cross_sum<double><<<g, blk, 0, st>>>(nrows, b, nslabs, (const double *)part, slab_stride, (double *)Y, ldy);
  else k_kernel_cross_sum<float><<<g, blk, 0, st>>>(nrows, b, nslabs, (const float *)part, slab_stride, (float *)Y, ldy);
}

}  // namespace slq
