// bf16 instantiations of the PDRF level networks' inference kernels, both levels (voxel_mlp_kernel.h).
#include "voxel_mlp_kernel.h"

namespace evd {

int launch_voxel_fwd_bf16(int HD, const VoxMlpParams& p, hipStream_t st) { return launch_voxel_fwd<EVD_PREC_BF16>(HD, p, st); }

}  // namespace evd
