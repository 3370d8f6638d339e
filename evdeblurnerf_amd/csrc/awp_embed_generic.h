// AWP sample embedding on float32 rows (evd_awp_api.hip evd_awp_embed_f32_*): AdaptiveWeightProposal.sample_feature_embed_layer, reference
// networks/dpnerf/awp.py:36-37,98-100, for the input widths of mode='nerf' -- run_nerf.py:223 builds the proposal with
// input_ch = netwidth, and the renderer hands it the NeRF network's per-sample feature (renderer.py:238-257).
// input_ch 64 / 128 / 256, width 64, depth 1..8.  Forward: one launch per layer of a float32 Linear + bias + ReLU on the matrix cores
// (gen_rows.h k_gen_linear_relu: v_mfma_f32_32x32x2f32, exact float32 products); every layer's output rows stay in the embedding's own
// store.  Backward: the per-layer launches of gen_rows.h (GenChain): no atomics, the same bits on every call.
#pragma once

#include "evd_common.h"
#include "gen_rows.h"

namespace evd {

constexpr int AWPG_MAX_D = 8;           // the width AWPG_W is the forward layer kernel's (gen_rows.h)
inline bool awpg_shape_ok(int input_ch, int width, int depth) {
    return (input_ch == 64 || input_ch == 128 || input_ch == 256) && width == AWPG_W && depth >= 1 && depth <= AWPG_MAX_D;
}

// The store: planes of float32 rows [nsp, 64], nsp = nsamp rounded up to the 32-sample tile.  Offsets in floats.
struct AwpGenStore {
    long nsp;
    int D;
    AwpGenStore(long nsamp, int D_) : nsp((nsamp + 31) / 32 * 32), D(D_) {}
    long h(int l) const { return nsp * AWPG_W * l; }            // ReLU output of layer l
    long g(int i) const { return nsp * AWPG_W * (D + i); }      // x 2: d loss / d pre-activation, ping-pong (what the backward writes)
    long total() const { return g(2); }
};

}  // namespace evd
