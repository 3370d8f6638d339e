// split-float16 instantiations of the PDRF level networks' inference kernels, both levels (voxel_mlp_kernel.h); the coarse level of
// an EVD_PREC_F16C render runs here too (p.rev_trig).
#include "voxel_mlp_kernel.h"

namespace evd {

int launch_voxel_fwd_f16x3(int HD, const VoxMlpParams& p, hipStream_t st) { return launch_voxel_fwd<EVD_PREC_F16X3>(HD, p, st); }

}  // namespace evd
