// fig_indel_kernel.hip -- the translation unit of fig_indel_kernel (fig_indel.h) and its launch.  It is kept out of
// fig_abi.hip's module so that the machine code of the kernels there is what it was before this one existed.
#include <hip/hip_runtime.h>
#define FIG_INDEL_KERNEL
#include "fig_indel.h"

hipError_t fig_indel_launch(const FigIndelArgs &A, unsigned items, hipStream_t stream) {
    hipLaunchKernelGGL(fig_indel_kernel, dim3(items), dim3(FIG_ID_NT), 0, stream, A);
    return hipGetLastError();
}
