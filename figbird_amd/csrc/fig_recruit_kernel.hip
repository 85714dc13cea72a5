// fig_recruit_kernel.hip -- the translation unit of fig_recruit_kernel (fig_recruit.h) and its launch.  It is kept out
// of fig_abi.hip's module so that the machine code of the kernels there is what it was before this one existed.
#include <hip/hip_runtime.h>
#define FIG_RECRUIT_KERNEL
#include "fig_recruit.h"

hipError_t fig_recruit_launch(const FigRecruitArgs &A, unsigned items, hipStream_t stream) {
    hipLaunchKernelGGL(fig_recruit_kernel, dim3(items), dim3(FIG_RC_NT), 0, stream, A);
    return hipGetLastError();
}
