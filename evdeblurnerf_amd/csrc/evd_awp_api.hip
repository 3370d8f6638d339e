// C-ABI entry points of the fused AWP sample-feature embedding: reference networks/dpnerf/awp.py:36-37 (the module list),
// :98-100 (its forward), trained by run_nerf.py:593-601.
#include "awp_embed.h"
#include "awp_embed_generic.h"
#include "evd_common.h"
#include "frag_layout.h"
#include "gen_rows.h"
#include "nerf_mlp.h"
#include "voxel_train.h"

#include <cstdint>

using namespace evd;

// the embedding on float32 rows (awp_embed_generic.h): the parameters as one float32 arena on the device, read in place by every launch
struct evd_awp_embed_f32 {
    int input_ch, depth;
    long param_off[2 * AWPG_MAX_D + 1];      // W0, b0, W1, b1, ...; [2 depth] = total
    DevBuf params;
};

struct evd_awp_embed {
    long param_off[2 * AWP_D + 1];           // W0, b0, W1, b1, ... in the flat parameter arena; [8] = total
    PackedStream fwd[2], bwd[2][AWP_D];      // [0] bf16, [1] f16
    DevBuf bias, bias_src, maps;
    RepackBatch batch;
};

static int prec_index(int precision) { return precision == EVD_PREC_BF16 ? 0 : (precision == EVD_PREC_F16 ? 1 : -1); }

extern "C" {

void evd_awp_embed_destroy(evd_awp_embed* a) {
    if (!a) return;
    for (int i = 0; i < 2; ++i) {
        a->fwd[i].release();
        for (int l = 0; l < AWP_D; ++l) a->bwd[i][l].release();
    }
    a->bias.release(); a->bias_src.release(); a->maps.release();
    a->batch.release();
    delete a;
}

int evd_awp_embed_create(const float* const* weights, const float* const* biases, int input_ch, int width, int depth, evd_awp_embed** out) {
    EVD_REQUIRE(weights && biases && out, "evd_awp_embed_create: null argument");
    EVD_REQUIRE(input_ch == AWP_IN && width == AWP_W && depth == AWP_D,
                "evd_awp_embed_create: built for input_ch %d, W_sam %d, D_sam %d (fine_geo_feat_dim / kernel_awp_sam_emb_* of the shipped configs), got %d / %d / %d",
                AWP_IN, AWP_W, AWP_D, input_ch, width, depth);
    for (int l = 0; l < AWP_D; ++l) EVD_REQUIRE(weights[l] && biases[l], "evd_awp_embed_create: missing layer %d", l);
    evd_awp_embed* a = new evd_awp_embed();
    ParamBlock blk[2 * AWP_D];
    for (int l = 0; l < AWP_D; ++l) {
        blk[2 * l] = {weights[l], (long)AWP_W * (l == 0 ? AWP_IN : AWP_W)};
        blk[2 * l + 1] = {biases[l], AWP_W};
    }
    const std::vector<float> arena = build_arena(blk, 2 * AWP_D, a->param_off);
    const float* A = arena.data();
    int rc = EVD_OK;
    for (int i = 0; i < 2 && !rc; ++i) {
        const int prec = i == 0 ? EVD_PREC_BF16 : EVD_PREC_F16;
        StreamBuilder sb = pipe_builder(prec, A);       // forward stream, the layer table of awp_embed_kernel.h AwpNet
        for (int l = 0; l < AWP_D; ++l) {
            const int in_dim = l == 0 ? AWP_IN : AWP_W;
            sb.layer(A + a->param_off[2 * l], AWP_W, in_dim, AWP_W / 32, in_dim / 16, l == AWP_D - 1, hid_col);
        }
        if ((long)sb.bytes.size() != (long)AWP_NCHUNKS * PIPE_CB) { evd_awp_embed_destroy(a); return fail(EVD_E_INVALID, "evd_awp_embed_create: stream geometry"); }
        rc = a->fwd[i].upload(sb);
        for (int l = 0; l < AWP_D && !rc; ++l) {        // W_l^T streams of the dgrad chain
            const int in_dim = l == 0 ? AWP_IN : AWP_W;
            rc = put_wt(a->bwd[i][l], prec, A, [&](StreamBuilder& b) {
                b.layer_transposed(A + a->param_off[2 * l], AWP_W, in_dim, 0, in_dim, nullptr, 0, in_dim / 32, AWP_W / 16, true, hid_col);
            });
        }
    }
    if (!rc) {
        BiasImage b(A, a->param_off);
        for (int l = 0; l < AWP_D; ++l) b.push(2 * l + 1, AWP_W, AWP_W / 32);
        rc = b.upload(a->bias, a->bias_src);
    }
    if (!rc) {
        std::vector<int> m(AMAP_TOTAL, -1);
        fill_map(m, AMAP_H, AWP_W, hid_col);
        fill_map(m, AMAP_GEO, AWP_IN, hid_col);
        rc = a->maps.upload(m.data(), m.size() * sizeof(int));
    }
    if (rc) { evd_awp_embed_destroy(a); return rc; }
    *out = a;
    return EVD_OK;
}

long evd_awp_embed_param_count(const evd_awp_embed* a) { return a ? a->param_off[2 * AWP_D] : 0; }

int evd_awp_embed_load_params(evd_awp_embed* a, const float* params, void* stream) {
    EVD_REQUIRE(a && params, "evd_awp_embed_load_params: null argument");
    hipStream_t st = as_stream(stream);
    int rc;
    std::vector<PackedStream*> all;
    for (int i = 0; i < 2; ++i) {
        all.push_back(&a->fwd[i]);
        for (int l = 0; l < AWP_D; ++l) all.push_back(&a->bwd[i][l]);
    }
    if ((rc = repack_batch(a->batch, all, params, st))) return rc;
    const long nb = (long)(a->bias.bytes / sizeof(float));
    hipLaunchKernelGGL(k_gather_f32, dim3((unsigned)cdiv(nb, 256L)), dim3(256), 0, st, params, (const int*)a->bias_src.p, nb, (float*)a->bias.p);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

size_t evd_awp_embed_store_bytes(const evd_awp_embed* a, long nsamp) {
    return (!a || nsamp < 0) ? 0 : (size_t)awp_tiles(nsamp) * awpstore::TILE_BYTES + awpstore::TRAILER_BYTES;
}

static const int AWP_WGRAD_BLOCKS = 256;
static const size_t AWP_WGRAD_PARTIAL_BYTES = (size_t)AWP_WGRAD_BLOCKS * 13 * 4096;      // the fused backward's 13 blocks per workgroup (awp_bwd_fused.h); a per-layer wgrad needs 2 x 5
size_t evd_awp_embed_backward_workspace_bytes(void) { WgradWs L; return wgrad_layout(AWP_WGRAD_PARTIAL_BYTES, nullptr, &L); }

int evd_awp_embed_forward(const evd_awp_embed* a, int precision, const float* geo_rows, const evd_voxel* fine, const void* fine_store,
                          size_t fine_store_bytes, long nsamp, float* h_local, void* store, size_t store_bytes, void* stream) {
    EVD_REQUIRE(a && h_local && nsamp >= 0, "evd_awp_embed_forward: null argument");
    const int pi = prec_index(precision);
    EVD_REQUIRE(pi >= 0, "evd_awp_embed_forward: built for precision f16 / bf16");
    EVD_REQUIRE((geo_rows != nullptr) != (fine_store != nullptr), "evd_awp_embed_forward: pass the geo features EITHER as float32 rows OR as the fine level's store");
    if (nsamp == 0) return EVD_OK;
    AwpFwdParams p;
    p.wstream = (const char*)a->fwd[pi].data.p; p.bias = (const float*)a->bias.p; p.geo_rows = geo_rows;
    p.geo_frags = nullptr; p.geo_tile_bytes = 0; p.geo_slot = 0;
    if (fine_store) {
        EVD_REQUIRE(fine, "evd_awp_embed_forward: the fine level's store needs the level handle");
        const size_t need = evd_voxel_train_store_bytes(fine, nsamp);      // half-precision layout: the level must have run in THIS precision
        EVD_REQUIRE(need > 0, "evd_awp_embed_forward: this level has no training store (only the standard fine level 256/128/64 with 2 + 3 layers trains); pass the geo features as float32 rows");
        EVD_REQUIRE(evd_voxel_geo_feat_dim(fine) == AWP_IN, "evd_awp_embed_forward: the level has %d geo channels, the embedding reads %d", evd_voxel_geo_feat_dim(fine), AWP_IN);
        if (fine_store_bytes < need) return fail(EVD_E_WORKSPACE, "evd_awp_embed_forward: fine store %zu < %zu bytes", fine_store_bytes, need);
        p.geo_frags = (const char*)fine_store; p.geo_tile_bytes = voxel_store_tile_bytes(256); p.geo_slot = voxel_store_geo_slot(256);
    }
    p.nsamp = nsamp; p.h_local = h_local; p.act = (char*)store; p.nchunks = AWP_NCHUNKS;
    if (store && store_bytes < evd_awp_embed_store_bytes(a, nsamp))
        return fail(EVD_E_WORKSPACE, "evd_awp_embed_forward: store %zu < %zu bytes", store_bytes, evd_awp_embed_store_bytes(a, nsamp));
    return precision == EVD_PREC_F16 ? launch_awp_embed_f16(store != nullptr, p, as_stream(stream)) : launch_awp_embed_bf16(store != nullptr, p, as_stream(stream));
}

int evd_awp_embed_backward(const evd_awp_embed* a, int precision, const float* d_h_local, long nsamp, void* store, size_t store_bytes,
                           const evd_awp_embed_grads* grads, float* d_geo_rows, const unsigned* d_h_absmax, void* workspace,
                           size_t workspace_bytes, void* stream) {
    EVD_REQUIRE(a && d_h_local && store && grads && workspace && nsamp >= 0, "evd_awp_embed_backward: null argument");
    const int pi = prec_index(precision);
    EVD_REQUIRE(pi >= 0, "evd_awp_embed_backward: built for precision f16 / bf16");
    if (nsamp == 0) return EVD_OK;
    if (store_bytes < evd_awp_embed_store_bytes(a, nsamp)) return fail(EVD_E_WORKSPACE, "evd_awp_embed_backward: store %zu < %zu bytes", store_bytes, evd_awp_embed_store_bytes(a, nsamp));
    WgradWs ws;
    const size_t need = wgrad_layout(AWP_WGRAD_PARTIAL_BYTES, workspace, &ws);
    if (workspace_bytes < need) return fail(EVD_E_WORKSPACE, "evd_awp_embed_backward: workspace %zu < %zu bytes", workspace_bytes, need);
    AwpBwdPlan b;
    b.d_h_local = d_h_local; b.d_h_absmax = d_h_absmax; b.nsamp = nsamp; b.tiles = awp_tiles(nsamp); b.store = (char*)store;
    for (int l = 0; l < AWP_D; ++l) {
        b.wt[l] = (const char*)a->bwd[pi][l].data.p;
        b.grads.w[l] = grads->w[l]; b.grads.b[l] = grads->b[l];
    }
    b.maps = (const int*)a->maps.p;
    b.partial = ws.partial;
    b.wgrad_blocks = AWP_WGRAD_BLOCKS;
    b.d_geo_rows = d_geo_rows;
    return precision == EVD_PREC_F16 ? run_awp_backward_f16(b, as_stream(stream)) : run_awp_backward_bf16(b, as_stream(stream));
}

// ---- float32 rows, input_ch 64 / 128 / 256 (awp_embed_generic.h) -------------------------------------------------------------------------

void evd_awp_embed_f32_destroy(evd_awp_embed_f32* a) {
    if (!a) return;
    a->params.release();
    delete a;
}

int evd_awp_embed_f32_create(const float* const* weights, const float* const* biases, int input_ch, int width, int depth, evd_awp_embed_f32** out) {
    EVD_REQUIRE(weights && biases && out, "evd_awp_embed_f32_create: null argument");
    EVD_REQUIRE(awpg_shape_ok(input_ch, width, depth), "evd_awp_embed_f32_create: built for input_ch 64 / 128 / 256, W_sam %d, D_sam 1..%d, got %d / %d / %d",
                AWPG_W, AWPG_MAX_D, input_ch, width, depth);
    for (int l = 0; l < depth; ++l) EVD_REQUIRE(weights[l] && biases[l], "evd_awp_embed_f32_create: missing layer %d", l);
    evd_awp_embed_f32* a = new evd_awp_embed_f32();
    a->input_ch = input_ch; a->depth = depth;
    ParamBlock blk[2 * AWPG_MAX_D];
    for (int l = 0; l < depth; ++l) {
        blk[2 * l] = {weights[l], (long)AWPG_W * (l == 0 ? input_ch : AWPG_W)};
        blk[2 * l + 1] = {biases[l], AWPG_W};
    }
    const std::vector<float> arena = build_arena(blk, 2 * depth, a->param_off);
    if (int rc = a->params.upload(arena.data(), arena.size() * sizeof(float))) { evd_awp_embed_f32_destroy(a); return rc; }
    *out = a;
    return EVD_OK;
}

long evd_awp_embed_f32_param_count(const evd_awp_embed_f32* a) { return a ? a->param_off[2 * a->depth] : 0; }

int evd_awp_embed_f32_load_params(evd_awp_embed_f32* a, const float* params, void* stream) {
    EVD_REQUIRE(a && params, "evd_awp_embed_f32_load_params: null argument");
    EVD_HIP(hipMemcpyAsync(a->params.p, params, a->params.bytes, hipMemcpyDeviceToDevice, as_stream(stream)));
    return EVD_OK;
}

size_t evd_awp_embed_f32_store_bytes(const evd_awp_embed_f32* a, long nsamp) {
    return (!a || nsamp < 0) ? 0 : (size_t)AwpGenStore(nsamp, a->depth).total() * sizeof(float);
}

size_t evd_awp_embed_f32_backward_workspace_bytes(void) { WgradWs L; return wgrad_layout(GEN_WS_FLOATS * sizeof(float), nullptr, &L); }

static bool rows_ok(const float* rows, long ld, int input_ch) { return ld >= input_ch && ld % 4 == 0 && ((uintptr_t)rows & 15) == 0; }

int evd_awp_embed_f32_forward(const evd_awp_embed_f32* a, const float* rows, long rows_stride, long nsamp, float* h_local, void* store,
                              size_t store_bytes, void* stream) {
    EVD_REQUIRE(a && rows && h_local && store && nsamp >= 0, "evd_awp_embed_f32_forward: null argument");
    EVD_REQUIRE(rows_ok(rows, rows_stride, a->input_ch), "evd_awp_embed_f32_forward: rows of %ld floats for %d channels (a multiple of 4, 16-byte aligned)",
                rows_stride, a->input_ch);
    if (nsamp == 0) return EVD_OK;
    const size_t need = evd_awp_embed_f32_store_bytes(a, nsamp);
    if (store_bytes < need) return fail(EVD_E_WORKSPACE, "evd_awp_embed_f32_forward: store %zu < %zu bytes", store_bytes, need);
    const AwpGenStore gs(nsamp, a->depth);
    float* S = (float*)store;
    const float* P = (const float*)a->params.p;
    for (int l = 0; l < a->depth; ++l) {
        GenLinear g;
        g.X = l == 0 ? rows : S + gs.h(l - 1); g.ldx = l == 0 ? rows_stride : AWPG_W;
        g.Wm = P + a->param_off[2 * l]; g.bias = P + a->param_off[2 * l + 1];
        g.out = S + gs.h(l); g.out2 = l == a->depth - 1 ? h_local : nullptr; g.nsamp = nsamp;
        if (int rc = launch_gen_linear_relu(l == 0 ? a->input_ch : AWPG_W, g, as_stream(stream))) return rc;
    }
    return EVD_OK;
}

int evd_awp_embed_f32_backward(const evd_awp_embed_f32* a, const float* d_h_local, const float* rows, long rows_stride, long nsamp, void* store,
                               size_t store_bytes, const evd_awp_embed_f32_grads* grads, float* d_rows, void* workspace, size_t workspace_bytes,
                               void* stream) {
    EVD_REQUIRE(a && d_h_local && rows && store && grads && workspace && nsamp >= 0, "evd_awp_embed_f32_backward: null argument");
    EVD_REQUIRE(rows_ok(rows, rows_stride, a->input_ch) && rows_stride <= INT32_MAX,
                "evd_awp_embed_f32_backward: rows of %ld floats for %d channels (a multiple of 4, 16-byte aligned)", rows_stride, a->input_ch);
    if (nsamp == 0) return EVD_OK;
    const size_t need_store = evd_awp_embed_f32_store_bytes(a, nsamp);
    if (store_bytes < need_store) return fail(EVD_E_WORKSPACE, "evd_awp_embed_f32_backward: store %zu < %zu bytes", store_bytes, need_store);
    WgradWs ws;
    const size_t need = wgrad_layout(GEN_WS_FLOATS * sizeof(float), workspace, &ws);
    if (workspace_bytes < need) return fail(EVD_E_WORKSPACE, "evd_awp_embed_f32_backward: workspace %zu < %zu bytes", workspace_bytes, need);
    hipStream_t st = as_stream(stream);
    const AwpGenStore gs(nsamp, a->depth);
    float* S = (float*)store;
    const float* P = (const float*)a->params.p;
    const int D = a->depth, W = AWPG_W;
    float *cur = S + gs.g(0), *oth = S + gs.g(1);
    // d pre-activation of the last layer: d h_local where its ReLU passed
    if (int rc = launch_gen_rows_in(d_h_local, W, S + gs.h(D - 1), nsamp, W, cur, st)) return rc;
    GenChain c{nsamp, ws.partial, 0, st, "evd_awp_embed_f32_backward"};
    for (int l = D - 1; l >= 0; --l) {          // cur = d pre-activation of layer l
        const float* wl = P + a->param_off[2 * l];
        if (l == 0) {
            c.wgrad(cur, W, W, rows, (int)rows_stride, a->input_ch, grads->w[0], a->input_ch, 0, grads->b[0]);
            if (d_rows) c.dgrad(W, cur, W, wl, a->input_ch, 0, a->input_ch, d_rows, a->input_ch, nullptr, 0, nullptr, nullptr, 0);
            break;
        }
        c.wgrad(cur, W, W, S + gs.h(l - 1), W, W, grads->w[l], W, 0, grads->b[l]);
        c.dgrad(W, cur, W, wl, W, 0, W, oth, W, S + gs.h(l - 1), W, nullptr, nullptr, 0);
        float* t = cur; cur = oth; oth = t;
    }
    return c.rc;
}

}  // extern "C"
