// C-ABI entry points of the PDRF backbone (reference networks/pdrf/voxnerf.py): a level's handle (voxel_net.h) -- create, destroy, and its
// network parameters.  Inference and the c2f renderer: evd_voxel_render_api.hip; network training: evd_voxel_train_api.hip; the grids as
// parameters: evd_voxel_grids_api.hip.
#include "voxel_net.h"
#include "voxel_streams.h"

#include <cmath>
#include <cstdint>
#include <cstdlib>

using namespace evd;

// the tri-plane grids of a level: planes / lines [1,C,H,W] -> channel-last [H][W][C], as float32 and as the float16 copy of the
// half-precision arithmetic modes (f16_sat of evd_common.h, as k_load_grids makes it), the basis, and the kernels' view of them (v->gp)
static int voxel_upload_grids(evd_voxel* v, const evd_voxel_desc* d) {
    int rc = EVD_OK;
    auto upload = [&](const float* src, int C, long n, DevBuf& f32, DevBuf& f16) {      // [C, n] -> channel-last [n][C]
        std::vector<float> cl((size_t)C * n);
        std::vector<_Float16> ch(cl.size());
        for (int c = 0; c < C; ++c)
            for (long k = 0; k < n; ++k) cl[(size_t)k * C + c] = src[(size_t)c * n + k];
        for (size_t k = 0; k < cl.size(); ++k) ch[k] = f16_sat(cl[k]);
        const int e = f32.upload(cl.data(), cl.size() * sizeof(float));
        return e ? e : f16.upload(ch.data(), ch.size() * sizeof(_Float16));
    };
    for (int i = 0; i < 3 && !rc; ++i) {
        v->n_comp[i] = d->n_comp[i]; v->grid[i] = d->grid[i];
        rc = upload(d->plane[i], d->n_comp[i], (long)d->grid[kMat0[i]] * d->grid[kMat1[i]], v->plane[i], v->plane_h[i]);
        if (!rc) rc = upload(d->line[i], d->n_comp[i], d->grid[kVec[i]], v->line[i], v->line_h[i]);
    }
    if (!rc) rc = v->basis.upload(d->basis, sizeof(float) * (size_t)d->app_dim * (d->n_comp[0] + d->n_comp[1] + d->n_comp[2]));
    if (!rc) rc = v->tv_acc.alloc((size_t)6 * 2 * TV_MAX_BLOCKS * sizeof(double));
    if (rc) return rc;
    GridParams& g = v->gp;
    for (int i = 0; i < 3; ++i) {
        g.plane[i] = (const float*)v->plane[i].p; g.line[i] = (const float*)v->line[i].p;
        g.plane_h[i] = (const _Float16*)v->plane_h[i].p; g.line_h[i] = (const _Float16*)v->line_h[i].p;
        g.n_comp[i] = d->n_comp[i]; g.grid[i] = d->grid[i];
        g.aabb_min[i] = d->aabb[i];
        g.inv[i] = 2.0f / (d->aabb[3 + i] - d->aabb[i]);
    }
    g.basis = (const float*)v->basis.p; g.app_dim = d->app_dim; g.app_act = d->app_act;
    return EVD_OK;
}

// the streams of mode prec (voxel_streams.h).  A generic level: the table of kernel_voxel_generic.hip in every mode, nothing else.  A
// standard level: the table of k_voxel_mlp where voxel_level_forward can select it, and in the pipelined modes of the standard encodings
// the VoxNet table (render and training forward) and the W^T streams of the backward
static int voxel_mode_streams(evd_voxel* v, int prec, const float* A, bool standard_enc) {
    int rc = EVD_OK;
    const bool piped = !v->generic && standard_enc && is_train_prec(prec);
    v->nchunks[prec] = v->fwd_chunks[prec] = 0;
    if (v->generic || has_generic_stream(piped, std_coarse(v))) {
        StreamBuilder sb(prec);
        sb.arena = A;
        if (v->generic) voxel_layers(sb, *v, A, VG_KF, VG_GK, true);
        else voxel_layers_legacy(sb, *v, A);
        v->nchunks[prec] = (int)(sb.bytes.size() / chunk_bytes(prec));
        if ((rc = v->stream[prec].upload(sb))) return rc;
    }
    if (!piped) return EVD_OK;
    StreamBuilder sp = pipe_builder(prec, A);
    voxel_layers(sp, *v, A, v->ft_dim / 16, 2 * ((v->geo + 31) / 32), false);
    v->fwd_chunks[prec] = (int)(sp.bytes.size() / PIPE_CB);
    if ((rc = v->fwd[prec].upload(sp))) return rc;
    return voxel_wt_streams(*v, prec, A);
}

extern "C" {

void evd_voxel_destroy(evd_voxel* v) {
    if (!v) return;
    for (int i = 0; i < 3; ++i) { v->plane[i].release(); v->line[i].release(); v->plane_h[i].release(); v->line_h[i].release(); }
    for (int i = 0; i < EVD_VOX_NUM_PREC; ++i) {
        v->stream[i].release(); v->fwd[i].release();
        for (int k = 0; k < VBWD_NSTREAMS; ++k) v->bwd[i][k].release();
    }
    v->basis.release(); v->bias.release(); v->bias_src.release(); v->tv_acc.release(); v->wmaps.release();
    v->pipe_c.release(); v->arena_dev.release(); v->cnet.release(); v->params_f32.release();
    v->side.release();
    v->batch.release();
    delete v;
}

int evd_voxel_create(const evd_voxel_desc* d, evd_voxel** out) {
    EVD_REQUIRE(d && out, "evd_voxel_create: null argument");
    // frequency counts other than (PE_L, PE_LV) run in the generic kernel only (inference; no pipelined / f16c / training streams)
    EVD_REQUIRE(d->multires >= 0 && d->multires <= PE_L_MAX && d->multires_views >= 0 && d->multires_views <= PE_LV,
                "evd_voxel_create: multires %d / multires_views %d out of range (0..%d / 0..%d)", d->multires, d->multires_views, PE_L_MAX, PE_LV);
    const int L = d->multires, Lv = d->multires_views;
    const bool standard = L == PE_L && Lv == PE_LV;
    const int NS = d->num_layers, NC = d->num_layers_color;
    EVD_REQUIRE(NS >= 1 && NS <= VG_MAX_LAYERS && NC >= 1 && NC <= VG_MAX_LAYERS,
                "evd_voxel_create: num_layers %d / num_layers_color %d out of range (1..%d each)", NS, NC, VG_MAX_LAYERS);
    const int IC = 3 * (1 + 2 * L), ICV = 3 * (1 + 2 * Lv);
    const int FT = d->input_ch - IC, HD = d->hidden_dim, G = d->geo_feat_dim;
    EVD_REQUIRE((HD == 64 || HD == 128 || HD == 256) && G >= 1 && G <= 32 * VG_GT && FT >= 16 && FT <= 16 * VG_KF && FT % 16 == 0,
                "evd_voxel_create: (hidden %d, geo %d, features %d) not built: hidden_dim 64, 128 or 256, geo_feat_dim 1..%d, "
                "input_ch - 3 (1 + 2 multires) a multiple of 16 in 16..%d", HD, G, FT, 32 * VG_GT, 16 * VG_KF);
    const bool generic = !voxel_standard_shape(NS, NC, HD, G, FT);
    EVD_REQUIRE(!generic || !d->composite_feature,
                "evd_voxel_create: composite_feature (kernel_type PBE) is built for the standard levels only (64/15/32 and 256/128/64 with 2 + 3 "
                "layers): its per-ray colour network is three layers");
    const int ctot = d->n_comp[0] + d->n_comp[1] + d->n_comp[2];
    EVD_REQUIRE(ctot <= 128 && d->n_comp[0] % 4 == 0 && d->n_comp[1] % 4 == 0 && d->n_comp[2] % 4 == 0 && d->app_dim <= 64,
                "evd_voxel_create: n_comp must be multiples of 4 with sum <= 128, app_dim <= 64");
    for (int i = 0; i < 3; ++i) EVD_REQUIRE(d->plane[i] && d->line[i] && d->grid[i] >= 1, "evd_voxel_create: missing grid %d", i);
    EVD_REQUIRE(d->basis, "evd_voxel_create: missing weights");
    for (int l = 0; l < NS; ++l) EVD_REQUIRE(d->sigma_w[l], "evd_voxel_create: missing weights (sigma_net.%d)", l);
    for (int l = 0; l < NC; ++l) EVD_REQUIRE(d->color_w[l], "evd_voxel_create: missing weights (color_net.%d)", l);

    evd_voxel* v = new evd_voxel();
    v->num_layers = NS; v->hidden_dim = HD; v->geo = G; v->num_layers_color = NC; v->input_ch = d->input_ch; v->ft_dim = FT;
    v->generic = generic; v->nblk = NS + 2 * NC;
    v->app_dim = d->app_dim; v->app_act = d->app_act; v->rgb_act = d->rgb_act; v->sigma_act = d->sigma_act;
    v->composite_feature = d->composite_feature ? 1 : 0; v->rmnear = d->rmnear;
    v->multires = L; v->multires_views = Lv;
    memcpy(v->aabb, d->aabb, sizeof(v->aabb));
    int rc = voxel_upload_grids(v, d);
    if (rc) { evd_voxel_destroy(v); return rc; }

    // The parameters in one host arena in the canonical order sigma_net.0 .., then color_net.l.{weight,bias} (a standard level:
    // sigma_net.0, sigma_net.1, color_net.{0,1,2}.{weight,bias}; a missing bias = zeros); every packed element records its arena index so
    // that evd_voxel_load_params can re-pack on the device (pack.h)
    ParamBlock blk[VG_MAX_LAYERS + 2 * VG_MAX_LAYERS];
    for (int l = 0; l < NS; ++l) blk[v->sigma_blk(l)] = {d->sigma_w[l], (long)(l == NS - 1 ? 1 + G : HD) * (l == 0 ? d->input_ch : HD)};
    for (int l = 0; l < NC; ++l) {
        const long outs = l == NC - 1 ? 3 : HD;
        blk[v->color_w_blk(l)] = {d->color_w[l], outs * (l == 0 ? G + ICV : HD)};
        blk[v->color_b_blk(l)] = {d->color_b[l], outs};
    }
    const std::vector<float> arena = build_arena(blk, v->nblk, v->param_off);
    const float* A = arena.data();
    if (v->composite_feature)       // the colour network runs per RAY on the composited features (voxnerf.py:231-239): plain float32 rows
        rc = v->cnet.upload(A + v->param_off[NS], (size_t)(v->param_off[v->nblk] - v->param_off[NS]) * sizeof(float));

    for (int prec = 0; prec < EVD_VOX_NUM_PREC && !rc; ++prec) rc = voxel_mode_streams(v, prec, A, standard);
    if (!rc && generic) rc = v->params_f32.upload(A, arena.size() * sizeof(float));     // read in place by the generic training backward
    if (!rc && !generic && standard && voxel_mlp_c_chunks(HD, G, FT) > 0) {
        StreamBuilderC sc(PIPE_CB);
        voxel_layers_c(sc, *v, A);
        v->pipe_c_chunks = (int)(sc.bytes.size() / PIPE_CB);
        if (v->pipe_c_chunks != voxel_mlp_c_chunks(HD, G, FT))
            rc = fail(EVD_E_INVALID, "evd_voxel_create: f16c stream has %d chunks, kernel expects %d", v->pipe_c_chunks, voxel_mlp_c_chunks(HD, G, FT));
        if (!rc) rc = v->pipe_c.upload(sc);
    }
    if (!rc && !generic) {
        const std::vector<int> m = voxel_wgrad_maps(*v);
        rc = v->wmaps.upload(m.data(), m.size() * sizeof(int));
    }
    if (!rc) {
        BiasImage b(A, v->param_off, 32 * 16);         // zero block shared by the bias-free sigma layers
        for (int l = 0; l < NC; ++l) b.push(v->color_b_blk(l), l == NC - 1 ? 3 : HD, l == NC - 1 ? 1 : HD / 32);
        rc = b.upload(v->bias, v->bias_src);
    }
    if (rc) { evd_voxel_destroy(v); return rc; }
    *out = v;
    return EVD_OK;
}

long evd_voxel_param_count(const evd_voxel* v) { return v ? v->param_off[v->nblk] : 0; }

int evd_voxel_param_blocks(const evd_voxel* v, long* offsets, int capacity) {
    EVD_REQUIRE(v, "evd_voxel_param_blocks: null level");
    if (offsets)
        for (int i = 0; i <= v->nblk && i < capacity; ++i) offsets[i] = v->param_off[i];
    return v->nblk;
}

int evd_voxel_load_params(evd_voxel* v, const float* params, void* stream) {
    EVD_REQUIRE(v && params, "evd_voxel_load_params: null argument");
    hipStream_t st = as_stream(stream);
    int rc;
    std::vector<PackedStream*> all;
    for (int i = 0; i < EVD_VOX_NUM_PREC; ++i) {
        all.push_back(&v->stream[i]);
        all.push_back(&v->fwd[i]);
        for (int k = 0; k < VBWD_NSTREAMS; ++k) all.push_back(&v->bwd[i][k]);
    }
    if ((rc = repack_batch(v->batch, all, params, st))) return rc;
    if (v->pipe_c_chunks > 0) {
        const size_t bytes = (size_t)v->param_off[v->nblk] * sizeof(float);
        if (!v->arena_dev.p && (rc = v->arena_dev.alloc(bytes))) return rc;
        EVD_HIP(hipMemcpyAsync(v->arena_dev.p, params, bytes, hipMemcpyDeviceToDevice, st));
        v->pipe_c_stale = true;
    }
    if (v->params_f32.p) EVD_HIP(hipMemcpyAsync(v->params_f32.p, params, v->params_f32.bytes, hipMemcpyDeviceToDevice, st));
    if (v->cnet.p) EVD_HIP(hipMemcpyAsync(v->cnet.p, params + v->param_off[v->num_layers], v->cnet.bytes, hipMemcpyDeviceToDevice, st));
    const long nb = (long)(v->bias.bytes / sizeof(float));
    hipLaunchKernelGGL(k_gather_f32, dim3((unsigned)cdiv(nb, 256L)), dim3(256), 0, st, params, (const int*)v->bias_src.p, nb, (float*)v->bias.p);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int evd_voxel_geo_feat_dim(const evd_voxel* v) { return v ? v->geo : 0; }

}  // extern "C"
