// The generic NeRF-mode training path (kernel_nerf_train_generic.hip): any view-branch network evd_nerf_mlp accepts, EVD_PREC_F16X3.
// reference: the autograd graph of networks/nerf.py:46-72,131-162 (NeRF.mlpforward + eval), embedding.py:88-98.
//
// Forward: k_nerf_mlp_generic's body in the split-float16 mode, with every layer's output also written as float32 rows.
// Backward: the per-layer kernels of gen_rows.h -- per layer one wgrad launch (per-wavefront partial sums over a sample range, folded in a
// fixed order by k_gen_wreduce) and one dgrad launch, both exact float32 products on the matrix cores (v_mfma_f32_32x32x2f32) with the
// parameters read in place from the handle's float32 copy.  No floating-point atomics, no host synchronisation.
// With a feature output (evd_nerf_mlp_train_feature / _backward_feature; every view-branch network, the pipelined 8 x 256 one included):
// the feature is a plane of the store (GenStore::f() or h(D - 1)), its gradient one more addend placed by k_gen_rows_in ahead of a dgrad
// that runs with `add`.
#pragma once

#include "evd_common.h"
#include "gen_rows.h"
#include "nerf_mlp.h"
#include "nerf_net.h"
#include "nerf_train.h"

namespace evd {

// The store: planes of float32 rows, nsp = nsamp rounded up to the 32-sample tile.  Offsets in floats.
struct GenStore {
    long nsp;
    int D, W;
    __host__ __device__ GenStore(long nsamp, int D_, int W_) : nsp((nsamp + 31) / 32 * 32), D(D_), W(W_) {}
    __host__ __device__ long in() const { return 0; }                              // [nsp, 8]: pts xyz, 0, viewdir xyz, 0
    __host__ __device__ long h(int l) const { return nsp * (8 + (long)l * W); }    // [nsp, W]: ReLU output of pts_linears[l]
    __host__ __device__ long f() const { return h(D); }                            // [nsp, W]: feature_linear output
    __host__ __device__ long hv() const { return h(D + 1); }                       // [nsp, W / 2]: ReLU output of views_linears.0
    // what the backward writes
    __host__ __device__ long g(int i) const { return hv() + nsp * (W / 2) + i * nsp * W; }   // [nsp, W] x 2: d loss / d pre-activation, ping-pong
    __host__ __device__ long enc(int i) const { return g(2) + i * nsp * GEN_ENC; }           // [nsp, 64] x 4: PE(pts), PE(dirs), d PE(pts), d PE(dirs)
    __host__ __device__ long total() const { return enc(4); }
};

// The entries with a feature output (evd_nerf_mlp_train_feature / evd_nerf_mlp_backward_feature) run these kernels for EVERY view-branch
// network, the 8 x 256 / (10, 4) / skips [4] one included; the plain entries only where the pipelined kernels are not built.
inline bool nerf_feature_trains(const evd_nerf* n, int prec) { return prec == EVD_PREC_F16X3 && !n->no_views && n->nchunks[EVD_PREC_F16X3] > 0; }
inline bool nerf_generic_trains(const evd_nerf* n, int prec) { return nerf_feature_trains(n, prec) && n->pipe_chunks[EVD_PREC_F16X3] == 0; }
inline size_t nerf_generic_store_bytes(const evd_nerf* n, long nsamp) { return (size_t)GenStore(nsamp, n->D, n->W).total() * sizeof(float); }

// pdh: the skip layer's k-step order of the stream in p (0 = the generic stream, evd_nerf::pd_pdh = evd_nerf::stream_pd)
int launch_nerf_train_fwd_generic(int W, const MlpParams& p, hipStream_t st, int pdh = 0);

struct GenBwdPlan {
    const evd_nerf* net;
    const float* d_raw;         // [nsamp, 4]
    long nsamp;
    float* store;
    float* partial;             // GEN_WS_FLOATS floats
    BwdGrads grads;
    int accumulate;
    float *d_pts, *d_dirs;      // [nsamp, 3] or null
    // d loss / d feature rows [nsamp, W] of ldf floats, or null: feature_kind 1 = the feature_linear output, 2 = the ReLU output of
    // pts_linears[D-1] (what the forward exposes as a plane of the store)
    const float* d_feature = nullptr;
    int ldf = 0, feature_kind = 0;
};
int run_nerf_backward_generic(const GenBwdPlan& b, hipStream_t st);

}  // namespace evd
