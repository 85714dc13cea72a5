// fig_indel_kernel.hip -- the translation unit of fig_indel_kernel (fig_indel.h) and its launch.  It is kept out of
// fig_abi.hip's module so that the machine code of the kernels there is what it was before this one existed.
#include <hip/hip_runtime.h>
#include "fig_placement_host.h"
#include "fig_readstage.h"
// fig_placement.h is wanted for fig_placement_column; it also defines fig_placement_kernel, which fig_abi.hip's module owns.  Inside
// an unnamed namespace the second definition is local to this unit: nothing refers to it and the host side drops it; this unit's code
// object carries an unused copy of it (1 400 instructions).
namespace {
#include "fig_placement.h"
}
#define FIG_INDEL_KERNEL
#include "fig_indel.h"

hipError_t fig_indel_launch(const FigIndelArgs &A, unsigned items, hipStream_t stream) {
    hipLaunchKernelGGL(fig_indel_kernel, dim3(items), dim3(FIG_ID_NT), 0, stream, A);
    return hipGetLastError();
}
