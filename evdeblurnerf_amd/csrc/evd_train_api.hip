// C-ABI entry points of the NeRF-mode training path: forward that keeps the activations, backward of the fused MLP
// (reference: the autograd graph of networks/nerf.py:46-72 NeRF.mlpforward, driven by run_nerf.py:593-601 loss.backward()).
#include "evd_common.h"
#include "nerf_mlp.h"
#include "nerf_net.h"
#include "nerf_train.h"
#include "nerf_train_generic.h"

#include <cstdint>
#include <cstdlib>

using namespace evd;

namespace evd {
constexpr int TRAIN_WG_SAMPLES = 256;       // samples per workgroup of the training kernels (8 wavefronts x 32)
static long train_tiles(long nsamp) { return cdiv(nsamp, (long)TRAIN_WG_SAMPLES) * (TRAIN_WG_SAMPLES / 32); }
// the mixed modes (include/evdnerf.h): EVD_PREC_F16C = compensated forward, EVD_PREC_F16M = split-float16 forward; both on the
// float16 mode's store and backward
static bool train_built(const evd_nerf* n, int prec) {
    if (prec == EVD_PREC_F16C) return n->pipe_chunks[EVD_PREC_F16] > 0 && n->pipe_chunks[EVD_PREC_F16C] > 0;
    if (prec == EVD_PREC_F16M) return n->pipe_chunks[EVD_PREC_F16] > 0 && n->pipe_chunks[EVD_PREC_F16X3] > 0;
    return prec >= 0 && prec < EVD_NUM_PREC && is_train_prec(prec) && n->pipe_chunks[prec] > 0;
}
static int store_prec(int prec) { return (prec == EVD_PREC_F16C || prec == EVD_PREC_F16M) ? EVD_PREC_F16 : prec; }
// what both entries say to a network / precision pair that neither path trains
#define EVD_TRAIN_REFUSAL(entry)                                                                                                              \
    entry ": the training path is built for precision f16 / bf16 / f16x3 / f16c / f16m on the netdepth 8, netwidth 256, skips [4] network; "  \
          "every other view-branch network trains in f16x3 only (use_viewdirs=False networks: not built)"
// and the entries with a per-sample feature output (the proposal's depth_feature, renderer.py:238-257): generic kernels only
#define EVD_FEATURE_REFUSAL(entry)                                                                                                      \
    entry ": the feature output under training is built for precision f16x3 on view-branch networks (use_viewdirs=False networks and "  \
          "every other precision: not built)"

// scratch of the backward (evd_common.h wgrad_layout): the wgrad partial sums of the largest block (8 x 9 accumulator tiles per wavefront group; generic: GEN_WS_FLOATS)
static const int WGRAD_BLOCKS = 256;
static size_t wgrad_partial_bytes(bool generic) { return generic ? GEN_WS_FLOATS * sizeof(float) : (size_t)WGRAD_BLOCKS * 8 * 9 * 4096; }
static size_t backward_ws_bytes(bool generic) { WgradWs L; return wgrad_layout(wgrad_partial_bytes(generic), nullptr, &L); }

// the caller's gradient pointers as the plans carry them
static BwdGrads plan_grads(const evd_nerf* net, const evd_nerf_grads* grads) {
    BwdGrads g;
    for (int l = 0; l < EVD_MAX_LAYERS; ++l) { g.pts_w[l] = l < net->D ? grads->pts_w[l] : nullptr; g.pts_b[l] = l < net->D ? grads->pts_b[l] : nullptr; }
    g.views_w = grads->views_w; g.views_b = grads->views_b; g.feature_w = grads->feature_w; g.feature_b = grads->feature_b;
    g.alpha_w = grads->alpha_w; g.alpha_b = grads->alpha_b; g.rgb_w = grads->rgb_w; g.rgb_b = grads->rgb_b;
    return g;
}

// The generic forward of `entry`: the generic inference kernel with stores, its encodings at run-time frequency counts.  pd: the pipelined
// network's stream with that kernel's order of additions in the skip layer, so that raw has the bits of evd_nerf_mlp_train.
static int train_fwd_generic(const char* entry, const evd_nerf* net, const float* ray_batch, const float* z, long R, int S, float* raw, void* store,
                             size_t store_bytes, bool pd, void* stream) {
    const size_t need = nerf_generic_store_bytes(net, R * (long)S);
    if (store_bytes < need) return fail(EVD_E_WORKSPACE, "%s: store %zu < %zu bytes", entry, store_bytes, need);
    MlpParams g = nerf_mlp_params(net, ray_batch, z, R, S, raw);
    g.wstream = (const char*)(pd ? net->stream_pd.data.p : net->stream[EVD_PREC_F16X3].data.p);
    g.nchunks = pd ? net->pd_chunks : net->nchunks[EVD_PREC_F16X3];
    g.act = (char*)store; g.pe_l = net->multires; g.pe_lv = net->multires_views;
    return launch_nerf_train_fwd_generic(net->W, g, as_stream(stream), pd ? net->pd_pdh : 0);
}

// The generic backward of `entry`; d_feature (rows of ldf floats, feature_kind 1 / 2) or null
static int backward_generic(const char* entry, const evd_nerf* net, const float* d_raw, const float* d_feature, int ldf, int feature_kind, long nsamp,
                            void* store, size_t store_bytes, const evd_nerf_grads* grads, float* d_pts, float* d_dirs, void* workspace,
                            size_t workspace_bytes, void* stream) {
    const size_t need_store = nerf_generic_store_bytes(net, nsamp);
    if (store_bytes < need_store) return fail(EVD_E_WORKSPACE, "%s: store %zu < %zu bytes", entry, store_bytes, need_store);
    WgradWs ws;
    const size_t need = wgrad_layout(wgrad_partial_bytes(true), workspace, &ws);
    if (workspace_bytes < need) return fail(EVD_E_WORKSPACE, "%s: workspace %zu < %zu bytes", entry, workspace_bytes, need);
    GenBwdPlan g;
    g.net = net; g.d_raw = d_raw; g.nsamp = nsamp; g.store = (float*)store;
    g.partial = ws.partial; g.grads = plan_grads(net, grads);
    g.accumulate = grads->accumulate ? 1 : 0; g.d_pts = d_pts; g.d_dirs = d_dirs;
    g.d_feature = d_feature; g.ldf = ldf; g.feature_kind = feature_kind;
    return run_nerf_backward_generic(g, as_stream(stream));
}
}  // namespace evd


extern "C" {

size_t evd_nerf_train_store_bytes(long nsamp) { return nsamp < 0 ? 0 : (size_t)train_tiles(nsamp) * astore::TILE_BYTES; }
size_t evd_nerf_train_store_bytes_prec(int precision, long nsamp) {
    const int sp = store_prec(precision);
    return (nsamp < 0 || sp < 0 || sp >= EVD_NUM_PREC || !is_train_prec(sp)) ? 0 : (size_t)train_tiles(nsamp) * astore::tile_bytes(sp);
}

size_t evd_nerf_train_feature_store_bytes(const evd_nerf* net, int precision, long nsamp) {
    return (net && nsamp >= 0 && nerf_feature_trains(net, precision)) ? nerf_generic_store_bytes(net, nsamp) : 0;
}
size_t evd_nerf_train_store_bytes_net(const evd_nerf* net, int precision, long nsamp) {
    if (!net || nsamp < 0) return 0;
    if (train_built(net, precision)) return evd_nerf_train_store_bytes_prec(precision, nsamp);
    return nerf_generic_trains(net, precision) ? evd_nerf_train_feature_store_bytes(net, precision, nsamp) : 0;
}

size_t evd_nerf_backward_workspace_bytes(void) { return backward_ws_bytes(false); }
size_t evd_nerf_backward_feature_workspace_bytes(const evd_nerf* net, int precision) {
    return (net && nerf_feature_trains(net, precision)) ? backward_ws_bytes(true) : 0;
}
size_t evd_nerf_backward_workspace_bytes_net(const evd_nerf* net, int precision) {
    if (!net) return 0;
    if (train_built(net, precision)) return backward_ws_bytes(false);
    return nerf_generic_trains(net, precision) ? evd_nerf_backward_feature_workspace_bytes(net, precision) : 0;
}

int evd_nerf_mlp_train(const evd_nerf* net, int precision, const float* ray_batch, const float* z, long R, int S, float* raw,
                       void* store, size_t store_bytes, void* stream) {
    EVD_REQUIRE(net && ray_batch && z && raw && store, "evd_nerf_mlp_train: null argument");
    const bool generic = !train_built(net, precision) && nerf_generic_trains(net, precision);
    EVD_REQUIRE(generic || train_built(net, precision), EVD_TRAIN_REFUSAL("evd_nerf_mlp_train"));
    EVD_REQUIRE(R >= 0 && S >= 1, "evd_nerf_mlp_train: bad shape R=%ld S=%d", R, S);
    if (R == 0) return EVD_OK;
    if (generic) return train_fwd_generic("evd_nerf_mlp_train", net, ray_batch, z, R, S, raw, store, store_bytes, false, stream);
    const long nsamp = R * (long)S;
    if (store_bytes < evd_nerf_train_store_bytes_prec(precision, nsamp))
        return fail(EVD_E_WORKSPACE, "evd_nerf_mlp_train: store %zu < %zu bytes", store_bytes, evd_nerf_train_store_bytes_prec(precision, nsamp));
    MlpParams p = nerf_mlp_params(net, ray_batch, z, R, S, raw);
    const int fwd = precision == EVD_PREC_F16M ? EVD_PREC_F16X3 : precision;      // the forward's stream
    p.wstream = (const char*)(fwd == EVD_PREC_F16C ? net->pipe_c.data.p : net->pipe[fwd].data.p);
    p.nchunks = net->pipe_chunks[fwd];
    p.act = (char*)store;
    if (precision == EVD_PREC_F16C) {
        p.wscale = (const unsigned*)net->pipe_c.scales.p;
        p.pe_l = PE_L; p.pe_lv = PE_LV;
        return launch_nerf_train_fwd_f16c(p, as_stream(stream));
    }
    if (precision == EVD_PREC_F16M) return launch_nerf_train_fwd_f16x3_hi(p, as_stream(stream));
    return precision == EVD_PREC_F16 ? launch_nerf_train_fwd_f16(p, as_stream(stream))
           : precision == EVD_PREC_BF16 ? launch_nerf_train_fwd_bf16(p, as_stream(stream)) : launch_nerf_train_fwd_f16x3(p, as_stream(stream));
}

int evd_nerf_mlp_backward(const evd_nerf* net, int precision, const float* d_raw, long R, int S, void* store, size_t store_bytes,
                          const evd_nerf_grads* grads, const float* pts, const float* viewdirs, int vd_stride, float* d_pts, float* d_dirs,
                          void* workspace, size_t workspace_bytes, void* stream) {
    EVD_REQUIRE((!d_pts || pts) && (!d_dirs || viewdirs), "evd_nerf_mlp_backward: d_pts / d_dirs need the forward's pts / viewdirs");
    EVD_REQUIRE(net && d_raw && store && grads && workspace, "evd_nerf_mlp_backward: null argument");
    const bool generic = !train_built(net, precision) && nerf_generic_trains(net, precision);
    EVD_REQUIRE(generic || train_built(net, precision), EVD_TRAIN_REFUSAL("evd_nerf_mlp_backward"));
    EVD_REQUIRE(R >= 0 && S >= 1, "evd_nerf_mlp_backward: bad shape R=%ld S=%d", R, S);
    if (R == 0) return EVD_OK;
    const long nsamp = R * (long)S;
    if (generic)
        return backward_generic("evd_nerf_mlp_backward", net, d_raw, nullptr, 0, 0, nsamp, store, store_bytes, grads, d_pts, d_dirs, workspace, workspace_bytes, stream);
    const size_t need_store = evd_nerf_train_store_bytes_prec(precision, nsamp);
    if (store_bytes < need_store) return fail(EVD_E_WORKSPACE, "evd_nerf_mlp_backward: store %zu < %zu bytes", store_bytes, need_store);
    WgradWs ws;
    const size_t need = wgrad_layout(wgrad_partial_bytes(false), workspace, &ws);
    if (workspace_bytes < need) return fail(EVD_E_WORKSPACE, "evd_nerf_mlp_backward: workspace %zu < %zu bytes", workspace_bytes, need);
    precision = store_prec(precision);          // the mixed modes: the float16 mode's store, W^T streams and kernels
    BwdPlan b;
    int rc0;
    b.d_raw = d_raw; b.nsamp = nsamp; b.tiles = train_tiles(nsamp); b.store = (char*)store;
    for (int k = 0; k < EVD_BWD_NSTREAMS; ++k) b.wt[k] = (const char*)net->bwd[precision][k].data.p;
    b.maps = (const int*)net->wmaps.p;
    b.maxbits = ws.maxbits; b.partial = ws.partial;
    b.wgrad_blocks = WGRAD_BLOCKS; b.skip = net->skip;
    // the wgrad launches run on the handle's side stream, forked from / joined to the caller's stream with events (stream order
    // as seen by the caller is unchanged): measured 3.41 -> 3.05 ms at 2^19 samples with 192 persistent wgrad workgroups
    // (256: 3.14, 128: 3.52).  EVD_BWD_OVERLAP=0 keeps everything on the caller's stream; =N sets the workgroup count (at most
    // WGRAD_BLOCKS, what the workspace is sized for).
    b.side = nullptr; b.ev = nullptr;
    if (const int nb = bwd_overlap_blocks(WGRAD_BLOCKS)) {
        if ((rc0 = net->side.get(&b.side, &b.ev))) return rc0;
        b.wgrad_blocks = nb;
    }
    b.pts = pts; b.viewdirs = viewdirs; b.vd_stride = vd_stride; b.S = S; b.d_pts = d_pts; b.d_dirs = d_dirs;
    b.grads = plan_grads(net, grads);
    b.accumulate = grads->accumulate ? 1 : 0;
    return precision == EVD_PREC_F16 ? run_nerf_backward_f16(b, as_stream(stream))
           : precision == EVD_PREC_BF16 ? run_nerf_backward_bf16(b, as_stream(stream)) : run_nerf_backward_f16x3(b, as_stream(stream));
}

int evd_nerf_mlp_train_feature(const evd_nerf* net, int precision, const float* ray_batch, const float* z, long R, int S, float* raw, int feature_kind,
                               void* store, size_t store_bytes, long* feature_offset, long* feature_stride, void* stream) {
    EVD_REQUIRE(net && ray_batch && z && raw && store && feature_offset && feature_stride, "evd_nerf_mlp_train_feature: null argument");
    EVD_REQUIRE(nerf_feature_trains(net, precision), EVD_FEATURE_REFUSAL("evd_nerf_mlp_train_feature"));
    EVD_REQUIRE(feature_kind == 1 || feature_kind == 2, "evd_nerf_mlp_train_feature: feature_kind %d (1 = after_linear, 2 = before_linear)", feature_kind);
    EVD_REQUIRE(R >= 0 && S >= 1, "evd_nerf_mlp_train_feature: bad shape R=%ld S=%d", R, S);
    const GenStore gs(R * (long)S, net->D, net->W);
    *feature_offset = feature_kind == 1 ? gs.f() : gs.h(net->D - 1);
    *feature_stride = net->W;
    if (R == 0) return EVD_OK;
    return train_fwd_generic("evd_nerf_mlp_train_feature", net, ray_batch, z, R, S, raw, store, store_bytes, net->pd_chunks > 0, stream);
}

int evd_nerf_mlp_backward_feature(const evd_nerf* net, int precision, const float* d_raw, const float* d_feature, long d_feature_stride, int feature_kind,
                                  long R, int S, void* store, size_t store_bytes, const evd_nerf_grads* grads, float* d_pts, float* d_dirs,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    EVD_REQUIRE(net && d_raw && store && grads && workspace, "evd_nerf_mlp_backward_feature: null argument");
    EVD_REQUIRE(nerf_feature_trains(net, precision), EVD_FEATURE_REFUSAL("evd_nerf_mlp_backward_feature"));
    EVD_REQUIRE(feature_kind == 1 || feature_kind == 2, "evd_nerf_mlp_backward_feature: feature_kind %d (1 = after_linear, 2 = before_linear)", feature_kind);
    EVD_REQUIRE(!d_feature || (d_feature_stride >= net->W && d_feature_stride <= INT32_MAX),
                "evd_nerf_mlp_backward_feature: d_feature rows of %ld floats, the feature has %d", d_feature_stride, net->W);
    EVD_REQUIRE(R >= 0 && S >= 1, "evd_nerf_mlp_backward_feature: bad shape R=%ld S=%d", R, S);
    if (R == 0) return EVD_OK;
    return backward_generic("evd_nerf_mlp_backward_feature", net, d_raw, d_feature, (int)d_feature_stride, feature_kind, R * (long)S, store, store_bytes,
                            grads, d_pts, d_dirs, workspace, workspace_bytes, stream);
}

}  // extern "C"
