// slq_kernelfeatureadj.hip — the instantiations of k_kernel_feature_adjoint (slq_kernelfeatureadj.hpp) in a
// translation unit of their own, so that the build stays parallel: 5 column widths in fp32 and 4 in fp64, each at 2 coordinate depths. The
// C-ABI over them (slq_kernel_feature_rmatmat / _rdmat) is in slq.hip and calls the launch function below; the slab partials are
// summed by kernel_cross_sum_launch (slq_kernelcross.hip).
#include <hip/hip_runtime.h>

#define SLQ_KERNELCROSS_DEVICE 1
#define SLQ_KERNELFEATURE_DEVICE 1
#include "slq_kernelfeatureadj.hpp"

namespace slq {

bool kernel_feature_adjoint_launch(int dtype_is_f64, const KernelSchedule &S, const KernelFeatureAdjArgs &a, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  return dtype_is_f64 ? kernel_feature_adjoint_launch_dtype<double>(S, a, st) : kernel_feature_adjoint_launch_dtype<float>(S, a, st);
}

}  // namespace slq
