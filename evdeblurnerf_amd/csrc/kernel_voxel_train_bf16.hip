// bf16 instantiations of the PDRF training kernels, both levels (voxel_mlp_kernel.h TRAIN variant, voxel_train_kernel.h).
#include "voxel_train_kernel.h"

namespace evd {

int launch_voxel_train_fwd_bf16(int HD, const VoxMlpParams& p, hipStream_t st) {
    if (HD == 256) return p.feature ? launch_voxel_train_fwd<EVD_PREC_BF16, 256, 128, 64, true>(p, st) : launch_voxel_train_fwd<EVD_PREC_BF16, 256, 128, 64>(p, st);
    if (p.feature) return launch_voxel_train_fwd64_rows<EVD_PREC_BF16>(p, st);      // (the 15 geo rows, read back out of the store)
    return launch_voxel_train_fwd<EVD_PREC_BF16, 64, 15, 32>(p, st);
}

int run_voxel_backward_bf16(int HD, const VoxBwdPlan& b, hipStream_t st) {
    return HD == 256 ? run_voxel_backward<EVD_PREC_BF16, 256, 128, 64>(b, st) : run_voxel_backward<EVD_PREC_BF16, 64, 15, 32>(b, st);
}

}  // namespace evd
