// C-ABI entry points of a PDRF level's network training: the level's sigma / colour networks, forward keeping the
// activation store and the hand-written backward, on the handle's streams (voxel_net.h).
#include "voxel_net.h"
#include "awp_embed.h"
#include "gen_rows.h"

using namespace evd;

extern "C" {

static const int VOX_WGRAD_BLOCKS = 256;
static long vox_tiles(long nsamp) { return cdiv(nsamp, 256L) * 8; }
// a generic level outside its one training mode: what both training entries answer
static int refuse_generic_mode(const evd_voxel* v, int precision, const char* entry) {
    EVD_REQUIRE(!v->generic || precision == EVD_PREC_F16X3, "%s: a level of this shape (hidden %d, geo %d, features %d, %d + %d layers) "
                "trains in precision f16x3 only; the other training modes are built for the standard levels (64/15/32 and 256/128/64 with 2 + 3 layers)",
                entry, v->hidden_dim, v->geo, v->ft_dim, v->num_layers, v->num_layers_color);
    return EVD_OK;
}

size_t evd_voxel_train_store_bytes(const evd_voxel* v, long nsamp) {
    return (!v || nsamp < 0 || v->generic) ? 0 : (size_t)vox_tiles(nsamp) * voxel_store_tile_bytes(v->hidden_dim);
}
size_t evd_voxel_train_store_bytes_prec(const evd_voxel* v, int precision, long nsamp) {
    if (!v || nsamp < 0 || !vox_train_built(v, precision)) return 0;
    if (v->generic) return (size_t)VoxGenStore(nsamp, v->hidden_dim, v->num_layers, v->num_layers_color).total() * sizeof(float);
    return (size_t)vox_tiles(nsamp) * voxel_store_tile_bytes_prec(v->hidden_dim, vox_store_prec(precision));
}

static const size_t VOX_WGRAD_PARTIAL_BYTES = (size_t)VOX_WGRAD_BLOCKS * 8 * 9 * 4096;
size_t evd_voxel_backward_workspace_bytes(void) { WgradWs L; return wgrad_layout(VOX_WGRAD_PARTIAL_BYTES, nullptr, &L); }
// a generic level: the wgrad partial sums of the generic path behind a 256-byte alignment
static const size_t VOX_GEN_WS_SLACK = 256;
size_t evd_voxel_backward_workspace_bytes_net(const evd_voxel* v, int precision) {
    if (!v) return 0;
    if (!v->generic) return evd_voxel_backward_workspace_bytes();
    return vox_train_built(v, precision) ? GEN_WS_FLOATS * sizeof(float) + VOX_GEN_WS_SLACK : 0;
}

int evd_voxel_mlp_train(const evd_voxel* v, int precision, const float* pts, const float* viewdirs, int vd_stride, const float* fts, int ft_stride,
                        long R, int S, float* raw, float* feature, void* store, size_t store_bytes, void* stream) {
    EVD_REQUIRE(v && pts && viewdirs && fts && raw && store, "evd_voxel_mlp_train: null argument");
    // a composite_feature level (kernel_type PBE) runs these kernels unchanged: raw and the geo rows before their activation leave as
    // `feature`, the composite and the colour network follow per ray (evd_raw2outputs_feat_bwd, evd_voxel_color_rows_train)
    EVD_REQUIRE(!v->composite_feature || (std_coarse(v) && (precision == EVD_PREC_F16X3 || precision == EVD_PREC_F16 || precision == EVD_PREC_BF16)),
                "evd_voxel_mlp_train: a composite_feature level trains as the standard coarse level (64/15/32) in precision f16x3 / f16 / bf16 "
                "(f16c / f16m keep no float32 feature rows)");
    if (const int rc = refuse_generic_mode(v, precision, "evd_voxel_mlp_train")) return rc;
    EVD_REQUIRE(vox_train_built(v, precision), "evd_voxel_mlp_train: the training path is built for precision f16 / bf16 / f16x3 / f16c / f16m");
    EVD_REQUIRE(R >= 0 && S >= 1 && ft_stride >= v->ft_dim && ft_stride % 4 == 0, "evd_voxel_mlp_train: bad shape");
    if (R == 0) return EVD_OK;
    const long nsamp = R * (long)S;
    if (store_bytes < evd_voxel_train_store_bytes_prec(v, precision, nsamp))
        return fail(EVD_E_WORKSPACE, "evd_voxel_mlp_train: store %zu < %zu bytes", store_bytes, evd_voxel_train_store_bytes_prec(v, precision, nsamp));
    VoxMlpParams p = vox_mlp_params(v, pts, viewdirs, vd_stride, fts, ft_stride, R, S, raw, feature, (char*)store);
    if (v->generic) {       // the generic inference kernel's body in the split-float16 mode, writing float32 rows: raw is the inference call's, bit for bit
        EVD_REQUIRE(vd_stride >= 3 && ((uintptr_t)store % 16) == 0, "evd_voxel_mlp_train: bad shape (the store 16-byte aligned)");
        p.pe_l = v->multires; p.pe_lv = v->multires_views;
        p.wstream = (const char*)v->stream[EVD_PREC_F16X3].data.p;
        p.nchunks = v->nchunks[EVD_PREC_F16X3];
        return voxel_train_fwd_generic_dispatch(v->hidden_dim, p, vox_gen_shape(v), as_stream(stream));
    }
    const bool mixed = precision == EVD_PREC_F16C || precision == EVD_PREC_F16M;      // a float32-grade forward writing the float16 mode's store
    if (mixed && feature) return fail(EVD_E_INVALID, "evd_voxel_mlp_train: float32 feature rows are not built in EVD_PREC_F16C / EVD_PREC_F16M (the geo features stay fragments in the store)");
    if (precision == EVD_PREC_F16C && v->pipe_c_chunks > 0) {        // the level's compensated kernel (fine level)
        int rc = use_pipe_c(v, p, as_stream(stream));
        return rc ? rc : launch_voxel_train_fwd_f16c(p, as_stream(stream));
    }
    const int arith = mixed ? EVD_PREC_F16X3 : precision;             // (vox_train_built: that stream exists)
    p.wstream = (const char*)v->fwd[arith].data.p;
    p.nchunks = v->fwd_chunks[arith];
    return mixed ? launch_voxel_train_fwd_f16x3_hi(v->hidden_dim, p, as_stream(stream))
                 : launch_voxel_train_fwd_dispatch(precision, v->hidden_dim, p, as_stream(stream));
}

int evd_voxel_mlp_backward(const evd_voxel* v, int precision, const float* d_raw, const float* raw, const float* d_feature, const void* awp_store,
                           size_t awp_store_bytes, long R, int S, void* store,
                           size_t store_bytes, const evd_voxel_grads* grads, float* d_fts, int d_fts_stride, const float* pts, const float* viewdirs, int vd_stride,
                           float* d_pts, float* d_dirs, void* workspace, size_t workspace_bytes, void* stream) {
    EVD_REQUIRE((!d_pts || pts) && (!d_dirs || viewdirs), "evd_voxel_mlp_backward: d_pts / d_dirs need the forward's pts / viewdirs");
    EVD_REQUIRE(v && d_raw && raw && store && grads && workspace, "evd_voxel_mlp_backward: null argument");
    if (const int rc = refuse_generic_mode(v, precision, "evd_voxel_mlp_backward")) return rc;
    EVD_REQUIRE(vox_train_built(v, precision), "evd_voxel_mlp_backward: the training path is built for precision f16 / bf16 / f16x3 / f16c / f16m");
    EVD_REQUIRE(R >= 0 && S >= 1 && (!d_fts || d_fts_stride >= v->ft_dim), "evd_voxel_mlp_backward: bad shape");
    if (R == 0) return EVD_OK;
    const long nsamp = R * (long)S;
    if (store_bytes < evd_voxel_train_store_bytes_prec(v, precision, nsamp))
        return fail(EVD_E_WORKSPACE, "evd_voxel_mlp_backward: store %zu < %zu bytes", store_bytes, evd_voxel_train_store_bytes_prec(v, precision, nsamp));
    if (v->generic) {
        EVD_REQUIRE(!awp_store, "evd_voxel_mlp_backward: awp_store goes with the f16 / bf16 modes of the standard fine level (pass the geo gradient as d_feature rows)");
        EVD_REQUIRE(((uintptr_t)store % 16) == 0, "evd_voxel_mlp_backward: the store must be 16-byte aligned");
        const size_t need = evd_voxel_backward_workspace_bytes_net(v, precision);
        if (workspace_bytes < need) return fail(EVD_E_WORKSPACE, "evd_voxel_mlp_backward: workspace %zu < %zu bytes", workspace_bytes, need);
        VoxGenBwdPlan b{};
        b.HD = v->hidden_dim; b.G = v->geo; b.FT = v->ft_dim; b.NS = v->num_layers; b.NC = v->num_layers_color; b.L = v->multires; b.Lv = v->multires_views;
        b.params = (const float*)v->params_f32.p; b.off = v->param_off;
        b.d_raw = d_raw; b.raw = raw; b.d_feature = d_feature; b.nsamp = nsamp; b.store = (float*)store; b.partial = (float*)ws_align_ptr(workspace);
        for (int l = 0; l < b.NS; ++l) b.sigma_w[l] = grads->sigma_w[l];
        for (int l = 0; l < b.NC; ++l) { b.color_w[l] = grads->color_w[l]; b.color_b[l] = grads->color_b[l]; }
        b.accumulate = grads->accumulate ? 1 : 0;
        b.d_fts = d_fts; b.d_fts_stride = d_fts_stride; b.d_pts = d_pts; b.d_dirs = d_dirs;
        return run_voxel_backward_generic(b, as_stream(stream));
    }
    WgradWs ws;
    const size_t need_ws = wgrad_layout(VOX_WGRAD_PARTIAL_BYTES, workspace, &ws);
    if (workspace_bytes < need_ws) return fail(EVD_E_WORKSPACE, "evd_voxel_mlp_backward: workspace %zu < %zu bytes", workspace_bytes, need_ws);
    precision = vox_store_prec(precision);      // EVD_PREC_F16C: the float16 mode's store, W^T streams and kernels
    VoxBwdPlan b;
    b.d_raw = d_raw; b.raw = raw; b.d_feature = d_feature; b.nsamp = nsamp; b.tiles = vox_tiles(nsamp); b.store = (char*)store;
    b.awp_store = nullptr; b.awp_tile_bytes = 0; b.awp_slot = 0; b.awp_words = nullptr;
    if (awp_store) {            // the fused AWP embedding ran its backward on this sample set: its d geo fragments join this level's
        const size_t need = (size_t)awp_tiles(nsamp) * awpstore::TILE_BYTES + awpstore::TRAILER_BYTES;
        EVD_REQUIRE(v->geo == AWP_IN, "evd_voxel_mlp_backward: awp_store goes with the fine level (geo %d)", AWP_IN);
        EVD_REQUIRE(is_half_prec(precision), "evd_voxel_mlp_backward: awp_store goes with the f16 / bf16 modes (in f16x3 pass the geo gradient as d_feature rows)");
        if (awp_store_bytes < need) return fail(EVD_E_WORKSPACE, "evd_voxel_mlp_backward: awp_store %zu < %zu bytes", awp_store_bytes, need);
        b.awp_store = (const char*)awp_store; b.awp_tile_bytes = awpstore::TILE_BYTES; b.awp_slot = awpstore::D_GEO;
        b.awp_words = (const unsigned*)(b.awp_store + awp_tiles(nsamp) * awpstore::TILE_BYTES);
    }
    for (int k = 0; k < VBWD_NSTREAMS; ++k) b.wt[k] = (const char*)v->bwd[precision][k].data.p;
    b.maps = (const int*)v->wmaps.p;
    b.maxbits = ws.maxbits; b.partial = ws.partial; b.wgrad_blocks = VOX_WGRAD_BLOCKS;
    b.side = nullptr; b.ev = nullptr;
    static const bool overlap = env_flag("EVD_BWD_OVERLAP_VOXEL");     // measured: no gain for the level networks (7.70 vs 7.86 ms per c2f iteration), off
    if (overlap) {
        if (const int nb = bwd_overlap_blocks(VOX_WGRAD_BLOCKS)) {
            int rc0 = v->side.get(&b.side, &b.ev);
            if (rc0) return rc0;
            b.wgrad_blocks = nb;
        }
    }
    b.d_fts = d_fts; b.d_fts_stride = d_fts_stride;
    b.pts = pts; b.viewdirs = viewdirs; b.vd_stride = vd_stride; b.S = S; b.d_pts = d_pts; b.d_dirs = d_dirs;
    for (int i = 0; i < 2; ++i) b.grads.sigma_w[i] = grads->sigma_w[i];
    for (int i = 0; i < 3; ++i) { b.grads.color_w[i] = grads->color_w[i]; b.grads.color_b[i] = grads->color_b[i]; }
    b.accumulate = grads->accumulate ? 1 : 0;
    return run_voxel_backward_dispatch(precision, v->hidden_dim, b, as_stream(stream));
}

}  // extern "C"
