// C-ABI entry points of a PDRF level's inference pass and of the mode='c2f' renderer (reference networks/pdrf/voxnerf.py,
// networks/renderer.py:182-217): the tri-plane gather, the level networks on the handle's streams (voxel_net.h), feature merging.
#include "voxel_net.h"
#include "voxel_color_rows.h"

using namespace evd;

extern "C" {

int evd_voxel_sample(const evd_voxel* v, const float* pts, long n, float* out, int out_stride, int out_col, void* stream) {
    EVD_REQUIRE(v && out && n >= 0 && out_stride >= out_col + v->app_dim, "evd_voxel_sample: bad arguments");
    if (n == 0) return EVD_OK;
    return launch_voxel_sample(v->gp, false, pts, n, out, out_stride, out_col, as_stream(stream));
}

static int sample_for(const evd_voxel* v, int precision, const float* pts, long n, float* out, int out_stride, int out_col, void* stream) {
    return launch_voxel_sample(v->gp, grids_half_for(v, precision), pts, n, out, out_stride, out_col, as_stream(stream));
}

int evd_voxel_sample_prec(const evd_voxel* v, int precision, const float* pts, long n, float* out, int out_stride, int out_col, void* stream) {
    EVD_REQUIRE(v && out && n >= 0 && out_stride >= out_col + v->app_dim, "evd_voxel_sample_prec: bad arguments");
    EVD_REQUIRE(precision >= 0 && precision <= EVD_PREC_F16M, "evd_voxel_sample_prec: unknown precision %d", precision);     // (F16M: the float32 grids)
    if (n == 0) return EVD_OK;
    return sample_for(v, precision, pts, n, out, out_stride, out_col, stream);
}

// composite_feature levels: the per-sample geo rows [R S, G] and the composited map [R, G] in the running entry's workspace (else nothing, null)
struct CompositeWs { float *rows = nullptr, *map = nullptr; };
static CompositeWs composite_layout(Workspace& ws, const evd_voxel* v, long R, int S) {
    if (!v->composite_feature) return {};
    float* rows = ws.take<float>((size_t)R * S * v->geo);
    return {rows, ws.take<float>((size_t)R * v->geo)};
}

struct VoxelForwardWs { float* raw; CompositeWs cs; };
static const size_t VOXEL_FORWARD_WS_SLACK = 512;       // alignment slack for an unaligned caller pointer plus the historical margin
static size_t voxel_forward_layout(const evd_voxel* v, long R, int S, void* workspace, VoxelForwardWs* L) {
    Workspace ws(workspace);
    L->raw = ws.take<float>((size_t)R * S * 4); L->cs = composite_layout(ws, v, R, S);
    return ws.used() + VOXEL_FORWARD_WS_SLACK;
}
size_t evd_voxel_forward_workspace_bytes(const evd_voxel* v, long R, int S) { VoxelForwardWs L; return (!v || R < 0 || S < 1) ? 0 : voxel_forward_layout(v, R, S, nullptr, &L); }

// activation of the geo rows before they are composited (voxnerf.py:172: rgb_activate(raw[..., 1:]))
static __global__ __launch_bounds__(256) void k_act_inplace(float* __restrict__ x, long n, int code) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) x[i] = act(code, x[i]);
}

// The network of a level's inference pass: picks the kernel and, with it, the stream of the handle it reads (p.wstream / p.nchunks).
static int voxel_level_forward(const evd_voxel* v, int precision, VoxMlpParams& p, hipStream_t st) {
    if (v->generic) {       // any other shape: its own kernel and stream in every mode; EVD_PREC_F16C runs float32-grade as on the standard coarse level
        const int prec = precision == EVD_PREC_F16C ? EVD_PREC_F16X3 : precision;
        p.wstream = (const char*)v->stream[prec].data.p;
        p.nchunks = v->nchunks[prec];
        return voxel_mlp_generic_dispatch(prec, v->hidden_dim, p, vox_gen_shape(v), st);
    }
    const bool coarse = std_coarse(v);
    bool coarse_of_f16c = false;
    if (precision == EVD_PREC_F16C) {
        if (v->pipe_c_chunks > 0) {     // the level's compensated kernel (standard fine level)
            if (p.feature) return fail(EVD_E_INVALID, "evd_voxel: per-sample feature rows are not built in EVD_PREC_F16C (use EVD_PREC_F16X3)");
            int rc = use_pipe_c(v, p, st);
            return rc ? rc : launch_voxel_pipe_f16c(p, st);
        }
        precision = EVD_PREC_F16X3;     // the standard coarse level: float32-grade arithmetic (a few % of the render)
        coarse_of_f16c = coarse;
    }
    // the pipelined stream of a standard level; the coarse level's kernels on it write no per-sample feature rows
    if (v->fwd_chunks[precision] > 0 && !(coarse && p.feature)) {
        p.wstream = (const char*)v->fwd[precision].data.p;
        p.nchunks = v->fwd_chunks[precision];
        p.rev_trig = coarse_of_f16c ? 1 : 0;       // an f16c render: this level's encodings as the fine level's kernel computes them (voxel_mlp_kernel.h)
        switch (precision) {
        case EVD_PREC_BF16: return launch_voxel_fwd_bf16(v->hidden_dim, p, st);
        case EVD_PREC_F16: return launch_voxel_fwd_f16(v->hidden_dim, p, st);
        case EVD_PREC_F16X3: return launch_voxel_fwd_f16x3(v->hidden_dim, p, st);
        }
    }
    // the generic kernel, any frequency counts: has_generic_stream() names exactly the levels and modes that arrive here
    if (!v->stream[precision].data.p)
        return fail(EVD_E_INVALID, "evd_voxel: no generic-layout stream for precision %d on this level (hidden %d, multires %d / %d)", precision,
                    v->hidden_dim, v->multires, v->multires_views);
    p.wstream = (const char*)v->stream[precision].data.p;
    p.nchunks = v->nchunks[precision];
    return voxel_mlp_dispatch(precision, v->hidden_dim, v->geo, v->ft_dim, p, st);
}

static int voxel_pass(const evd_voxel* v, int precision, const float* pts, const float* viewdirs, int vd_stride, const float* fts,
                      int ft_stride, const float* z, const float* rays_d, int rd_stride, long R, int S, int is_train,
                      const float* noise, float* color, float* depth, float* acc, float* weights, float* feature, float* raw,
                      void* stream, const CompositeWs& cs = {}) {
    // composite_feature (PBE, voxnerf.py:223-239): the per-sample geo rows are composited, the colour network runs per ray; `feature`
    // is then the composited map [R, G] (NULL: not wanted) and cs holds the rows + the map
    float *crows = nullptr, *cmap = nullptr;
    if (v->composite_feature) {
        if (!cs.rows) return fail(EVD_E_WORKSPACE, "evd_voxel: a composite_feature level needs its scratch (workspace sized by the *_workspace_bytes query of this handle)");
        crows = cs.rows;
        cmap = feature ? feature : cs.map;
        feature = crows;
    }
    VoxMlpParams p = vox_mlp_params(v, pts, viewdirs, vd_stride, fts, ft_stride, R, S, raw, feature, nullptr);
    p.pe_l = v->multires; p.pe_lv = v->multires_views;
    int rc = voxel_level_forward(v, precision, p, as_stream(stream));
    if (rc) return rc;
    const float thr = (!is_train && v->rmnear > 0.f) ? (float)((double)v->rmnear / 128.0) : 0.f;
    if (v->composite_feature) {
        hipStream_t st = as_stream(stream);
        const long ng = R * (long)S * v->geo;
        if (v->rgb_act != EVD_ACT_NONE) {
            hipLaunchKernelGGL(k_act_inplace, dim3((unsigned)cdiv(ng, 256L)), dim3(256), 0, st, crows, ng, v->rgb_act);
            EVD_LAUNCH_CHECK();
        }
        // weights / depth / acc from the densities; the geo rows ride along as the feature map (sum_s w feature); the per-sample colour
        // composite written to `color` here is overwritten by the per-ray colour network below
        if ((rc = evd_raw2outputs(raw, z, rays_d, rd_stride, R, S, 4, 0, 1, 3, v->rgb_act, v->sigma_act, 0, thr, noise,
                                  color, nullptr, acc, weights, depth, crows, v->geo, cmap, stream))) return rc;
        hipLaunchKernelGGL(k_color_rows<false>, dim3((unsigned)cdiv(R, 4L)), dim3(256), 0, st, (const float*)v->cnet.p, cmap, viewdirs, vd_stride, R, v->geo,
                           v->hidden_dim, v->multires_views, color, (float*)nullptr, (float*)nullptr);
        EVD_LAUNCH_CHECK();
        return EVD_OK;
    }
    return evd_raw2outputs(raw, z, rays_d, rd_stride, R, S, 4, 0, 1, 3, v->rgb_act, v->sigma_act, 0, thr, noise,
                           color, nullptr, acc, weights, depth, nullptr, 0, nullptr, stream);
}

int evd_voxel_forward(const evd_voxel* v, int precision, const float* pts, const float* viewdirs, int vd_stride, const float* fts, int F,
                      const float* z, const float* rays_d, int rays_d_stride, long R, int S, int is_train,
                      float* color, float* depth, float* acc, float* weights, float* feature,
                      void* workspace, size_t workspace_bytes, void* stream) {
    EVD_REQUIRE(v && pts && viewdirs && fts && z && rays_d, "evd_voxel_forward: null argument");
    EVD_REQUIRE(precision >= 0 && precision <= EVD_PREC_F16C, "evd_voxel_forward: unknown precision %d", precision);
    EVD_REQUIRE(F == v->ft_dim, "evd_voxel_forward: fts has %d channels, this level takes %d", F, v->ft_dim);
    EVD_REQUIRE(weights, "evd_voxel_forward: the weights output is required");
    if (R == 0) return EVD_OK;
    VoxelForwardWs L;
    const size_t need = voxel_forward_layout(v, R, S, workspace, &L);
    if (!workspace || workspace_bytes < need) return fail(EVD_E_WORKSPACE, "evd_voxel_forward: workspace %zu < %zu bytes", workspace_bytes, need);
    return voxel_pass(v, precision, pts, viewdirs, vd_stride, fts, F, z, rays_d, rays_d_stride, R, S, is_train, nullptr,
                      color, depth, acc, weights, feature, L.raw, stream, L.cs);
}

int evd_voxel_mlp(const evd_voxel* v, int precision, const float* pts, const float* viewdirs, int vd_stride, const float* fts, int ft_stride,
                  long R, int S, float* raw, float* feature, void* stream) {
    EVD_REQUIRE(v && pts && viewdirs && fts && raw, "evd_voxel_mlp: null argument");
    EVD_REQUIRE(precision >= 0 && precision <= EVD_PREC_F16C, "evd_voxel_mlp: unknown precision %d", precision);
    EVD_REQUIRE(R >= 0 && S >= 1 && vd_stride >= 3 && ft_stride >= v->ft_dim && ft_stride % 4 == 0, "evd_voxel_mlp: bad shape (fts rows of at least %d floats, a multiple of 4)", v->ft_dim);
    if (R == 0) return EVD_OK;
    VoxMlpParams p = vox_mlp_params(v, pts, viewdirs, vd_stride, fts, ft_stride, R, S, raw, feature, nullptr);
    p.pe_l = v->multires; p.pe_lv = v->multires_views;
    return voxel_level_forward(v, precision, p, as_stream(stream));
}

// The workspace of evd_c2f_render and evd_c2f_render_rays: slot 0 is the ray batch evd_c2f_render packs
struct C2fRenderWs { float *rb, *z0, *z2, *pts, *ft, *ft0, *ftn, *ptn; int* order; float *raw, *wts0, *wts, *zs; CompositeWs cs0, cs1; };
static const size_t C2F_RENDER_WS_SLACK = 512;          // alignment slack for an unaligned caller pointer plus the historical margin
static size_t c2f_render_layout(const evd_voxel* coarse, const evd_voxel* fine, const evd_render_cfg* cfg, long R, void* workspace, C2fRenderWs* L) {
    const size_t S = cfg->N_samples, Ni = cfg->N_importance > 0 ? cfg->N_importance : 0, St = S + Ni, Nn = Ni ? Ni : 1, r = (size_t)R;
    Workspace ws(workspace);
    L->rb = ws.take<float>(r * 11); L->z0 = ws.take<float>(r * S);
    L->z2 = ws.take<float>(r * St);             // z merged
    L->pts = ws.take<float>(r * St * 3);
    L->ft = ws.take<float>(r * St * 64);        // features [n,64]
    L->ft0 = ws.take<float>(r * S * 32);        // coarse features at the coarse samples [R*S,32]
    L->ftn = ws.take<float>(r * Nn * 32);       // coarse features at the new samples
    L->ptn = ws.take<float>(r * Nn * 3);        // new points
    L->order = ws.take<int>(r * St);            // sort order
    L->raw = ws.take<float>(r * St * 4); L->wts0 = ws.take<float>(r * S); L->wts = ws.take<float>(r * St);
    L->zs = ws.take<float>(r * Nn);             // z_samples
    L->cs0 = composite_layout(ws, coarse, R, (int)S);      // a composite_feature level (kernel_type PBE): geo rows + composited map
    L->cs1 = (fine && Ni) ? composite_layout(ws, fine, R, (int)St) : CompositeWs{};
    return ws.used() + C2F_RENDER_WS_SLACK;
}

size_t evd_c2f_render_workspace_bytes(const evd_voxel* coarse, const evd_voxel* fine, const evd_render_cfg* cfg, long R) {
    C2fRenderWs L;
    return (!coarse || !cfg || R < 0) ? 0 : c2f_render_layout(coarse, fine, cfg, R, nullptr, &L);
}

int evd_c2f_render_rays(const evd_voxel* coarse, const evd_voxel* fine, const evd_render_cfg* cfg, const float* rb, long R,
                        const float* t_rand, const float* u, const float* noise0, const float* noise1,
                        evd_render_out* out, void* workspace, size_t workspace_bytes, void* stream) {
    EVD_REQUIRE(coarse && cfg && out && (rb || R == 0), "evd_c2f_render_rays: null argument");
    EVD_REQUIRE(cfg->use_viewdirs, "evd_c2f_render_rays: use_viewdirs=False is not supported");
    EVD_REQUIRE(cfg->N_importance <= 0 || fine, "evd_c2f_render_rays: N_importance > 0 needs the fine level");
    EVD_REQUIRE(cfg->N_importance <= 0 || cfg->N_samples >= 3, "evd_c2f_render_rays: hierarchical sampling needs N_samples >= 3");
    EVD_REQUIRE(!(cfg->perturb > 0.f) || (t_rand && (cfg->N_importance <= 0 || u)), "evd_c2f_render_rays: perturb > 0 needs explicit draws");
    EVD_REQUIRE(coarse->ft_dim == coarse->app_dim && (!fine || fine->ft_dim == coarse->app_dim + fine->app_dim),
                "evd_c2f_render_rays: feature widths do not chain (coarse app_dim %d, fine input %d)", coarse->app_dim, fine ? fine->ft_dim : -1);
    if (R == 0) return EVD_OK;
    C2fRenderWs L;
    const size_t need = c2f_render_layout(coarse, fine, cfg, R, workspace, &L);
    if (!workspace || workspace_bytes < need) return fail(EVD_E_WORKSPACE, "evd_c2f_render_rays: workspace %zu < %zu bytes", workspace_bytes, need);
    const int S = cfg->N_samples, Ni = cfg->N_importance > 0 ? cfg->N_importance : 0, St = S + Ni;
    hipStream_t st = as_stream(stream);
    float *z0 = L.z0, *z2 = L.z2, *pts = L.pts, *ft = L.ft, *ft0 = L.ft0, *ftn = L.ftn, *ptn = L.ptn, *raw = L.raw, *wts0 = L.wts0, *wts = L.wts, *zs = L.zs;
    const int FS = 64;      // feature row stride: coarse features at column 0, fine at column coarse->app_dim (renderer.py:195)
    int rc;
    float* zc = (Ni ? (out->z_vals0 ? out->z_vals0 : z0) : (out->z_vals ? out->z_vals : z0));
    if ((rc = launch_sample_z_pts(cfg, rb, 11, R, t_rand, zc, pts, st))) return rc;       // z stratification + pts = o + d z (renderer.py:163-180)
    const int FC = coarse->app_dim;
    EVD_REQUIRE(!Ni || (FC == 32 && FC % 4 == 0), "evd_c2f_render_rays: coarse app_dim %d (workspace is sized for 32)", FC);
    EVD_REQUIRE(FC <= FS && (!Ni || !fine || FC + fine->app_dim <= FS),
                "evd_c2f_render_rays: app_dim %d + %d exceeds the feature row stride %d", FC, (Ni && fine) ? fine->app_dim : 0, FS);
    if (!Ni) {
        if ((rc = sample_for(coarse, cfg->precision, pts, R * (long)S, ft, FS, 0, stream))) return rc;      // renderer.py:183
        float* wo = out->weights ? out->weights : wts;
        return voxel_pass(coarse, cfg->precision, pts, rb + 8, 11, ft, FS, zc, rb + 3, 11, R, S, cfg->is_train, noise0,
                          out->rgb, out->depth, out->acc, wo, out->feature, out->raw ? out->raw : raw, stream, L.cs0);
    }
    if ((rc = sample_for(coarse, cfg->precision, pts, R * (long)S, ft0, FC, 0, stream))) return rc;          // renderer.py:183
    float* w0 = out->weights0 ? out->weights0 : wts0;
    if ((rc = voxel_pass(coarse, cfg->precision, pts, rb + 8, 11, ft0, FC, zc, rb + 3, 11, R, S, cfg->is_train, noise0,
                         out->rgb0, out->depth0, out->acc0, w0, nullptr, raw, stream, L.cs0))) return rc;
    float* zm = out->z_vals ? out->z_vals : z2;
    // (+ the positions of the new and of the merged samples: the coarse pass is done with `pts`)
    if ((rc = launch_sample_pdf_merge_pts(zc, w0, R, S, Ni, cfg->perturb == 0.f, u, zs, zm, L.order, out->z_std, rb, 11, ptn, pts, st))) return rc;
    // merged sample set (renderer.py:205-213), as the reference does it: coarse features are sampled at the NEW points only
    // (:209) and the rows of the old and new points are gathered by the sort order (:212-213); the fine level is sampled at
    // all merged points (:211 samples the new ones and :194 the old ones -- a pure function of the point either way).
    const long n2 = R * (long)St;
    if ((rc = sample_for(coarse, cfg->precision, ptn, R * (long)Ni, ftn, FC, 0, stream))) return rc;
    if ((rc = launch_merge_features(ft0, ftn, L.order, R, S, Ni, FC, ft, FS, st))) return rc;
    if ((rc = sample_for(fine, cfg->precision, pts, n2, ft, FS, coarse->app_dim, stream))) return rc;
    float* wo = out->weights ? out->weights : wts;
    return voxel_pass(fine, cfg->precision, pts, rb + 8, 11, ft, FS, zm, rb + 3, 11, R, St, cfg->is_train, noise1,
                      out->rgb, out->depth, out->acc, wo, out->feature, out->raw ? out->raw : raw, stream, L.cs1);
}

int evd_c2f_render(const evd_voxel* coarse, const evd_voxel* fine, const evd_render_cfg* cfg, const float* rays, long R,
                   const float* t_rand, const float* u, const float* noise0, const float* noise1,
                   evd_render_out* out, void* workspace, size_t workspace_bytes, void* stream) {
    EVD_REQUIRE(cfg && coarse && (rays || R == 0), "evd_c2f_render: null argument");
    if (R == 0) return EVD_OK;
    C2fRenderWs L;
    const size_t need = c2f_render_layout(coarse, fine, cfg, R, workspace, &L);
    if (!workspace || workspace_bytes < need) return fail(EVD_E_WORKSPACE, "evd_c2f_render: workspace %zu < %zu bytes", workspace_bytes, need);
    int rc = evd_ray_batch(cfg, rays, R, L.rb, stream);
    if (rc) return rc;
    return evd_c2f_render_rays(coarse, fine, cfg, L.rb, R, t_rand, u, noise0, noise1, out, workspace, workspace_bytes, stream);
}

// ---- the coarse feature rows of the merged sample set (renderer.py:209-213), as an operation of its own for the training path
int evd_merge_features(const float* old, const float* fresh, const int* order, long R, int S, int N, int F, float* out, int out_stride, void* stream) {
    EVD_REQUIRE(old && fresh && order && out && R >= 0 && S >= 1 && N >= 1 && F >= 4 && F % 4 == 0 && out_stride >= F && out_stride % 4 == 0,
                "evd_merge_features: bad arguments (F and out_stride multiples of 4)");
    if (R == 0) return EVD_OK;
    return launch_merge_features(old, fresh, order, R, S, N, F, out, out_stride, as_stream(stream));
}

int evd_merge_features_bwd(const float* d_out, int d_stride, const int* order, long R, int S, int N, int F, float* d_old, float* d_fresh, void* stream) {
    EVD_REQUIRE(d_out && order && d_old && d_fresh && R >= 0 && S >= 1 && N >= 1 && F >= 4 && F % 4 == 0 && d_stride >= F && d_stride % 4 == 0,
                "evd_merge_features_bwd: bad arguments (F and d_stride multiples of 4)");
    if (R == 0) return EVD_OK;
    return launch_merge_features_bwd(d_out, d_stride, order, R, S, N, F, d_old, d_fresh, as_stream(stream));
}

}  // extern "C"
