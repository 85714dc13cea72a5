// fig_alnqual_kernel.hip -- the translation unit of fig_alnqual_path_kernel and fig_alnqual_column_kernel (fig_alnqual.h; DESIGN.md
// §5i) and their launches.  It is kept out of fig_abi.hip's module so that the machine code of the kernels there is what it was before
// these existed.
#include <hip/hip_runtime.h>
#define FIG_ALNQUAL_KERNEL
#include "fig_alnqual.h"

hipError_t fig_alnqual_path_launch(const FigAlnPathArgs &A, unsigned items, hipStream_t stream) {
    hipLaunchKernelGGL(fig_alnqual_path_kernel, dim3(items), dim3(FIG_AQ_NT), 0, stream, A);
    return hipGetLastError();
}

hipError_t fig_alnqual_column_launch(const FigAlnColArgs &A, unsigned gaps, hipStream_t stream) {
    hipLaunchKernelGGL(fig_alnqual_column_kernel, dim3(gaps), dim3(FIG_AQ_NT), 0, stream, A);
    return hipGetLastError();
}
