// fig_polish_kernel.hip -- the translation unit of fig_polish_kernel (fig_polish.h) and its launch.  It is kept out
// of fig_abi.hip's module so that the machine code of the kernels there is what it was before this one existed.
#include <hip/hip_runtime.h>
#define FIG_POLISH_KERNEL
#include "fig_polish.h"

hipError_t fig_polish_launch(const FigPolishArgs &A, unsigned items, hipStream_t stream) {
    hipLaunchKernelGGL(fig_polish_kernel, dim3(items), dim3(FIG_ID_NT), 0, stream, A);
    return hipGetLastError();
}
