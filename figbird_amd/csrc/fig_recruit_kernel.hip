// fig_recruit_kernel.hip -- the translation unit of fig_recruit_kernel (fig_recruit.h) and its launch.  It is kept out
// of fig_abi.hip's module so that the machine code of the kernels there is what it was before this one existed.
#include <hip/hip_runtime.h>
#include "fig_placement_host.h"
#include "fig_readstage.h"
// As in fig_indel_kernel.hip: fig_placement.h is wanted for fig_placement_column, fig_placement_score and the wave reductions and
// also defines fig_placement_kernel, which fig_abi.hip's module owns; inside an unnamed namespace the second definition is local to
// this unit and nothing refers to it.
namespace {
#include "fig_placement.h"
}
#define FIG_RECRUIT_KERNEL
#include "fig_recruit.h"

hipError_t fig_recruit_launch(const FigRecruitArgs &A, unsigned items, hipStream_t stream) {
    hipLaunchKernelGGL(fig_recruit_kernel, dim3(items), dim3(FIG_RC_NT), 0, stream, A);
    return hipGetLastError();
}
