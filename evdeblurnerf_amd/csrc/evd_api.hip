#include <atomic>
// C-ABI entry points of the NeRF backbone: weight packing, fused MLP launch, render_rays orchestration.
#include "evd_common.h"
#include "nerf_mlp.h"
#include "nerf_mlp_kernel.h"
#include "nerf_net.h"
#include "nerf_streams.h"
#include "nerf_train.h"
#include "nerf_train_generic.h"
#include "pack.h"

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace evd {

char* err_buf() {
    static thread_local char buf[512] = {0};
    return buf;
}

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err_buf(), 512, fmt, ap);
    va_end(ap);
    return code;
}

int nerf_mlp_generic_dispatch(int prec, int W, const MlpParams& p, hipStream_t st);
int nerf_mlp_pipe_dispatch(int prec, const MlpParams& p, hipStream_t st);
int nerf_mlp_c_dispatch(int W, int D, int skip, const MlpParams& p, hipStream_t st);       // kernel_nerf_mlp.hip: compensated float16 mode
int nerf_mlp_c_chunks(int W, int D, int skip, bool train);                                 // 0: not built for this network; train: the unfolded stream

// Inference in the compensated mode folds feature_linear (no activation, read by views_linears.0 only) into the views layer:
//     Wfold = [Wv[:, :W] Wf | Wv[:, W:]]  (W/2 x (W + ICV)),   bfold = Wv[:, :W] bf + bv
// written behind a device copy of the parameter arena (evd_nerf::fold_arena) that the folded stream's re-pack maps index.  Every
// element is ONE float64 fma chain over k = 0 .. W-1 in that order, rounded once to float32: creation and re-pack run this kernel, so
// their streams agree bit for bit.  thread = one element of Wfold (row-major), then of bfold.
static __global__ void k_fold_feature(const float* __restrict__ views_w, const float* __restrict__ views_b, const float* __restrict__ feature_w,
                                      const float* __restrict__ feature_b, int W, int ICV, float* __restrict__ wfold, float* __restrict__ bfold) {
    const int in = W + ICV, rows = W / 2;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < (long)rows * in) {
        const int r = (int)(i / in), c = (int)(i % in);
        if (c >= W) { wfold[i] = views_w[i]; return; }
        double acc = 0.0;
        for (int k = 0; k < W; ++k) acc = fma((double)views_w[(long)r * in + k], (double)feature_w[(long)k * W + c], acc);
        wfold[i] = (float)acc;
    } else if (i < (long)rows * in + rows) {
        const int r = (int)(i - (long)rows * in);
        double acc = 0.0;
        for (int k = 0; k < W; ++k) acc = fma((double)views_w[(long)r * in + k], (double)feature_b[k], acc);
        bfold[r] = (float)(acc + (double)views_b[r]);
    }
}

// the folded stream, its row scales and its bias block from the parameter values at `params` (device, canonical order): one path for
// evd_nerf_create and evd_nerf_load_params
static int nerf_fold_pack(evd_nerf* n, const float* params, hipStream_t st) {
    if (!n->pipe_cf.data.p) return EVD_OK;
    const int W = n->W, D = n->D, ICV = 3 * (1 + 2 * n->multires_views);
    const long total = n->param_off[n->nparam_blocks], nw = (long)(W / 2) * (W + ICV), nel = nw + W / 2;
    float* ext = (float*)n->fold_arena.p;
    EVD_HIP(hipMemcpyAsync(ext, params, (size_t)total * sizeof(float), hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k_fold_feature, dim3((unsigned)cdiv(nel, 256L)), dim3(256), 0, st, ext + n->param_off[2 * D], ext + n->param_off[2 * D + 1],
                       ext + n->param_off[2 * D + 2], ext + n->param_off[2 * D + 3], W, ICV, ext + total, ext + total + nw);
    EVD_LAUNCH_CHECK();
    int rc = repack_stream_c(n->pipe_cf, ext, st);
    if (rc) return rc;
    const long nb = (long)(n->bias_f.bytes / sizeof(float));
    hipLaunchKernelGGL(k_gather_f32, dim3((unsigned)cdiv(nb, 256L)), dim3(256), 0, st, (const float*)ext, (const int*)n->bias_f_src.p, nb, (float*)n->bias_f.p);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

// the side-stream test hook (evd_common.h): ONE copy of the spin kernel in the library, the launch checked, launches counted
static std::atomic<long> g_side_spins{0};
static __global__ void k_test_spin(long long ticks) {          // wall_clock64: the constant 100 MHz counter
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}
int test_side_spin(hipStream_t side) {
    static const int us = [] { const char* e = getenv("EVD_TEST_SIDE_SPIN_US"); return e ? atoi(e) : 0; }();
    if (us <= 0) return EVD_OK;
    hipLaunchKernelGGL(k_test_spin, dim3(1), dim3(64), 0, side, (long long)us * 100);
    EVD_LAUNCH_CHECK();
    g_side_spins.fetch_add(1, std::memory_order_relaxed);
    return EVD_OK;
}
bool test_skip_side_join() {
    static const bool skip = [] { const char* e = getenv("EVD_TEST_SKIP_SIDE_JOIN"); return e && e[0] == '1'; }();
    return skip;
}

}  // namespace evd

using namespace evd;

extern "C" {

const char* evd_last_error(void) { return evd::err_buf(); }
long evd_debug_side_spin_count(void) { return evd::g_side_spins.load(std::memory_order_relaxed); }
int evd_version(void) { return 130; }      // 130: evd_nerf_train_store_bytes_net, evd_nerf_backward_workspace_bytes_net (generic NeRF training path, netwidth 128); 110: training entries (evd_*_train, evd_*_backward, evd_*_load_params, ...); 120: evd_awp_embed_*, the f16x3 training mode (evd_*_train_store_bytes_prec), evd_voxel_mlp_backward(awp_store), evd_voxel_sample_bwd_ws, evd_merge_features

int evd_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return fail(EVD_E_NODEVICE, "hipGetDeviceCount failed");
    return n;
}

// Every stream keeps, next to its bytes, the index map element -> parameter arena (pack.h), so that new parameter values
// are re-packed on the device (evd_nerf_load_params) with the arithmetic the host packer used at creation.

// canonical parameter order of the arena: pts_linears[l].{weight, bias} for l < D, then views_linears.0, feature_linear,
// alpha_linear, rgb_linear ({weight, bias} each; a missing bias = zeros); use_viewdirs=False: then output_linear.{weight, bias}.  Returns the
// number of blocks
static int nerf_param_blocks(const evd_nerf_desc* d, bool no_views, ParamBlock* blk) {
    const int D = d->D, W = d->W, IC = 3 * (1 + 2 * d->multires), ICV = 3 * (1 + 2 * d->multires_views);
    for (int l = 0; l < D; ++l) {
        blk[2 * l] = {d->pts_w[l], (long)W * (l == 0 ? IC : (l - 1 == d->skip ? W + IC : W))};
        blk[2 * l + 1] = {d->pts_b[l], W};
    }
    ParamBlock* h = blk + 2 * D;
    if (no_views) {
        h[NB_OUTPUT] = {d->output_w, (long)d->output_ch * W}; h[NB_OUTPUT + 1] = {d->output_b, d->output_ch};
        return 2 * D + 2;
    }
    h[NB_VIEWS] = {d->views_w, (long)(W / 2) * (W + ICV)}; h[NB_VIEWS + 1] = {d->views_b, W / 2};
    h[NB_FEATURE] = {d->feature_w, (long)W * W}; h[NB_FEATURE + 1] = {d->feature_b, W};
    h[NB_ALPHA] = {d->alpha_w, W}; h[NB_ALPHA + 1] = {d->alpha_b, 1};
    h[NB_RGB] = {d->rgb_w, 3L * (W / 2)}; h[NB_RGB + 1] = {d->rgb_b, 3};
    return 2 * D + 8;
}

// compensated float16 mode: its own streams (float16 + fp6 fragments) and row scales, pipelined kernel only -- the training forward's
// (pipe_c) and the folded inference stream (pipe_cf), whose builder gives the layout and the maps over zeros: the values are always filled
// on the device (nerf_fold_pack)
static int nerf_streams_c(evd_nerf* n, const float* A) {
    const int W = n->W, D = n->D, prec = EVD_PREC_F16C;
    StreamBuilderC sc(PIPE_CB);
    nerf_layers_c(sc, *n, A, false);
    n->pipe_chunks[prec] = (int)(sc.bytes.size() / PIPE_CB);
    if (n->pipe_chunks[prec] != nerf_mlp_c_chunks(W, D, n->skip, true))
        return fail(EVD_E_INVALID, "evd_nerf_create: f16c stream has %d chunks, kernel expects %d", n->pipe_chunks[prec], nerf_mlp_c_chunks(W, D, n->skip, true));
    int rc = n->pipe_c.upload(sc);
    if (rc) return rc;
    const long total = n->param_off[n->nparam_blocks], nfold = (long)(W / 2) * (W + 3 * (1 + 2 * n->multires_views)) + W / 2;
    std::vector<float> ext((size_t)(total + nfold), 0.f);
    StreamBuilderC sf(PIPE_CB);
    nerf_layers_c(sf, *n, ext.data(), true);
    n->fold_chunks = (int)(sf.bytes.size() / PIPE_CB);
    if (n->fold_chunks != nerf_mlp_c_chunks(W, D, n->skip, false))
        return fail(EVD_E_INVALID, "evd_nerf_create: folded f16c stream has %d chunks, kernel expects %d", n->fold_chunks, nerf_mlp_c_chunks(W, D, n->skip, false));
    rc = n->pipe_cf.upload(sf);
    return rc ? rc : n->fold_arena.alloc(ext.size() * sizeof(float));
}

int evd_nerf_create(const evd_nerf_desc* d, evd_nerf** out) {
    EVD_REQUIRE(d && out, "evd_nerf_create: null argument");
    // frequency counts other than (PE_L, PE_LV) run in the generic kernel only (no pipelined / f16c / training streams)
    EVD_REQUIRE(d->multires >= 0 && d->multires <= PE_L_MAX && d->multires_views >= 0 && pe_ksteps(d->multires_views) <= 4,
                "evd_nerf_create: multires %d / multires_views %d out of range (0..%d / 0..10)", d->multires, d->multires_views, PE_L_MAX);
    const bool standard = d->multires == PE_L && d->multires_views == PE_LV;
    EVD_REQUIRE(d->W == 256 || d->W == 128 || d->W == 64, "evd_nerf_create: netwidth %d not built (64, 128, 256)", d->W);
    EVD_REQUIRE(d->D >= 1 && d->D <= EVD_MAX_LAYERS, "evd_nerf_create: netdepth %d out of range", d->D);
    const bool no_views = !d->views_w && !d->feature_w && !d->alpha_w && !d->rgb_w && d->output_w;
    EVD_REQUIRE(no_views || (d->views_w && d->feature_w && d->alpha_w && d->rgb_w),
                "evd_nerf_create: give either the view branch (views / feature / alpha / rgb) or output_linear (use_viewdirs=False)");
    EVD_REQUIRE(!no_views || (d->output_b && (d->output_ch == 4 || d->output_ch == 5)), "evd_nerf_create: output_linear needs its bias and output_ch 4 or 5");
    const int W = d->W, KS = W / 16, D = d->D;
    evd_nerf* n = new evd_nerf();
    n->multires = d->multires; n->multires_views = d->multires_views;
    n->D = D; n->W = W; n->skip = d->skip; n->rgb_act = d->rgb_act; n->sigma_act = d->sigma_act; n->rmnear = d->rmnear;
    n->no_views = no_views ? 1 : 0;

    // host copy of every parameter in one arena; the packers read from it
    ParamBlock blk[2 * EVD_MAX_LAYERS + 8];
    n->nparam_blocks = nerf_param_blocks(d, no_views, blk);
    const std::vector<float> arena = build_arena(blk, n->nparam_blocks, n->param_off);
    const float* A = arena.data();
    const int out_rows = d->output_ch < 4 ? d->output_ch : 4;       // raw2outputs reads channels 0..3

    int rc = EVD_OK;
    for (int prec = 0; prec < EVD_NUM_PREC && !rc; ++prec) {
        n->nchunks[prec] = n->pipe_chunks[prec] = 0;
        if (prec == EVD_PREC_F16C) {
            if (!no_views && standard && nerf_mlp_c_chunks(W, D, d->skip, false)) rc = nerf_streams_c(n, A);
            continue;
        }
        StreamBuilder sb(prec);
        sb.arena = A;
        nerf_layers(sb, *n, A, out_rows, 0);
        n->nchunks[prec] = (int)(sb.bytes.size() / chunk_bytes(prec));
        rc = n->stream[prec].upload(sb);
        if (!rc && !no_views && standard && nerf_pipe_built(prec, W, D, d->skip)) {
            StreamBuilder sp = pipe_builder(prec, A, nerf_group(prec));
            nerf_layers(sp, *n, A, out_rows, KS - 2 * nerf_group(prec));
            n->pipe_chunks[prec] = (int)(sp.bytes.size() / PIPE_CB);
            rc = n->pipe[prec].upload(sp);
        }
        if (!rc && prec == EVD_PREC_F16X3 && n->pipe_chunks[prec]) {        // (see nerf_net.h stream_pd)
            StreamBuilder sd(prec);
            sd.arena = A;
            n->pd_pdh = KS - 2 * nerf_group(prec);
            nerf_layers(sd, *n, A, out_rows, n->pd_pdh);
            n->pd_chunks = (int)(sd.bytes.size() / chunk_bytes(prec));
            rc = n->stream_pd.upload(sd);
        }
        // training path (bf16 / f16 / split-f16 on the pipelined network)
        if (!rc && is_train_prec(prec) && n->pipe_chunks[prec]) rc = nerf_wt_streams(*n, prec, A);
    }
    if (!rc) {
        const std::vector<int> m = nerf_wgrad_maps(*n);
        rc = n->wmaps.upload(m.data(), m.size() * sizeof(int));
    }
    if (rc) { evd_nerf_destroy(n); return rc; }
    const BiasImage b = nerf_bias_image(*n, A, out_rows);
    rc = b.upload(n->bias, n->bias_src);
    if (!rc && n->pipe_cf.data.p) {      // folded f16c stream: its bias block (no feature tiles, bfold as the views bias), then the device fill
        const int T = W / 32;
        const long total = n->param_off[n->nparam_blocks], nw = (long)(W / 2) * (W + 3 * (1 + 2 * n->multires_views));
        std::vector<int32_t> fsrc(b.src.begin(), b.src.begin() + (D * T + 1) * 32);
        for (int i = 0; i < (T / 2) * 32; ++i) fsrc.push_back((int32_t)(total + nw + i));
        fsrc.insert(fsrc.end(), b.src.end() - 32, b.src.end());
        rc = n->bias_f_src.upload(fsrc.data(), fsrc.size() * sizeof(int32_t));
        if (!rc) rc = n->bias_f.alloc(fsrc.size() * sizeof(float));
        DevBuf dev_params;
        if (!rc) rc = dev_params.upload(arena.data(), arena.size() * sizeof(float));
        if (!rc) rc = nerf_fold_pack(n, (const float*)dev_params.p, nullptr);
        if (!rc && hipStreamSynchronize(nullptr) != hipSuccess) rc = fail(EVD_E_HIP, "evd_nerf_create: the folded f16c stream could not be packed");
        dev_params.release();
    }
    // generic training path (nerf_train_generic.h): its backward reads the float32 parameters in place
    // (every view-branch network: the entries with a feature output run that path for the pipelined network too)
    if (!rc && nerf_feature_trains(n, EVD_PREC_F16X3)) rc = n->params_f32.upload(arena.data(), arena.size() * sizeof(float));
    if (rc) { evd_nerf_destroy(n); return rc; }
    *out = n;
    return EVD_OK;
}

void evd_nerf_destroy(evd_nerf* n) {
    if (!n) return;
    for (int i = 0; i < EVD_NUM_PREC; ++i) {
        n->stream[i].release();
        n->pipe[i].release();
        for (int k = 0; k < EVD_BWD_NSTREAMS; ++k) n->bwd[i][k].release();
    }
    n->stream_pd.release();
    n->wmaps.release();
    n->batch.release();
    n->bias.release();
    n->bias_src.release();
    n->pipe_c.release();
    n->pipe_cf.release();
    n->bias_f.release();
    n->bias_f_src.release();
    n->fold_arena.release();
    n->params_f32.release();
    n->side.release();
    delete n;
}

long evd_nerf_param_count(const evd_nerf* net) { return net ? net->param_off[net->nparam_blocks] : 0; }

int evd_nerf_param_blocks(const evd_nerf* net, long* offsets, int capacity) {
    EVD_REQUIRE(net, "evd_nerf_param_blocks: null network");
    if (offsets)
        for (int i = 0; i <= net->nparam_blocks && i < capacity; ++i) offsets[i] = net->param_off[i];
    return net->nparam_blocks;
}

int evd_nerf_load_params(evd_nerf* net, const float* params, void* stream) {
    EVD_REQUIRE(net && params, "evd_nerf_load_params: null argument");
    hipStream_t st = as_stream(stream);
    int rc;
    std::vector<PackedStream*> all;
    for (int i = 0; i < EVD_NUM_PREC; ++i) {
        all.push_back(&net->stream[i]);
        all.push_back(&net->pipe[i]);
        for (int k = 0; k < EVD_BWD_NSTREAMS; ++k) all.push_back(&net->bwd[i][k]);
    }
    all.push_back(&net->stream_pd);
    if ((rc = repack_batch(net->batch, all, params, st))) return rc;
    if ((rc = repack_stream_c(net->pipe_c, params, st))) return rc;
    const long nb = (long)(net->bias.bytes / sizeof(float));
    hipLaunchKernelGGL(k_gather_f32, dim3((unsigned)cdiv(nb, 256L)), dim3(256), 0, st, params, (const int*)net->bias_src.p, nb, (float*)net->bias.p);
    EVD_LAUNCH_CHECK();
    if (net->params_f32.p) EVD_HIP(hipMemcpyAsync(net->params_f32.p, params, net->params_f32.bytes, hipMemcpyDeviceToDevice, st));
    return nerf_fold_pack(net, params, st);
}

size_t evd_nerf_stream_bytes(const evd_nerf* net, int precision) {
    if (!net || precision < 0 || precision >= EVD_NUM_PREC) return 0;
    if (precision == EVD_PREC_F16C) return net->pipe_cf.data.bytes;       // the stream the inference launch reads (the training forward: pipe_c)
    return net->pipe_chunks[precision] ? net->pipe[precision].data.bytes : net->stream[precision].data.bytes;
}

int evd_nerf_mlp(const evd_nerf* net, int precision, const float* ray_batch, const float* z, long R, int S,
                 float* raw, float* feature, int feature_kind, void* stream) {
    EVD_REQUIRE(net && ray_batch && z && raw, "evd_nerf_mlp: null argument");
    EVD_REQUIRE(precision >= 0 && precision < EVD_NUM_PREC, "evd_nerf_mlp: unknown precision %d", precision);
    EVD_REQUIRE(R >= 0 && S >= 1, "evd_nerf_mlp: bad shape R=%ld S=%d", R, S);
    EVD_REQUIRE(!feature || feature_kind == 1 || feature_kind == 2, "evd_nerf_mlp: feature_kind must be 1 or 2");
    if (R == 0) return EVD_OK;
    EVD_REQUIRE(!(net->no_views && feature && feature_kind == 1), "evd_nerf_mlp: a use_viewdirs=False network has no after_linear feature (nerf.py:159)");
    EVD_REQUIRE(!net->no_views || precision != EVD_PREC_F16C, "evd_nerf_mlp: EVD_PREC_F16C is not built for use_viewdirs=False networks");
    MlpParams p = nerf_mlp_params(net, ray_batch, z, R, S, raw);
    const bool piped = net->pipe_chunks[precision] > 0;
    p.wstream = (const char*)(piped ? net->pipe[precision].data.p : net->stream[precision].data.p);
    p.nchunks = piped ? net->pipe_chunks[precision] : net->nchunks[precision];
    p.no_views = net->no_views; p.pe_l = net->multires; p.pe_lv = net->multires_views;
    p.feature = feature; p.feature_kind = feature ? feature_kind : 0;
    if (precision == EVD_PREC_F16C) {
        EVD_REQUIRE(net->pipe_chunks[precision] > 0, "evd_nerf_mlp: EVD_PREC_F16C is built for netdepth 8, netwidth 256, skips [4], multires 10 / 4 only");
        EVD_REQUIRE(!feature, "evd_nerf_mlp: EVD_PREC_F16C has no feature-row variant (use EVD_PREC_F16X3)");
        p.wstream = (const char*)net->pipe_cf.data.p;       // feature_linear folded into the views layer
        p.nchunks = net->fold_chunks;
        p.wscale = (const unsigned*)net->pipe_cf.scales.p;
        p.bias = (const float*)net->bias_f.p;
        p.nbias = (int)(net->bias_f.bytes / sizeof(float));
        return nerf_mlp_c_dispatch(net->W, net->D, net->skip, p, as_stream(stream));
    }
    if (piped) return nerf_mlp_pipe_dispatch(precision, p, as_stream(stream));
    return nerf_mlp_generic_dispatch(precision, net->W, p, as_stream(stream));
}

// ------------------------------------------------------------------------------------------------
// NeRFAll.render + render_rays, mode='nerf' (networks/renderer.py:399-466, 129-264 else-branch).  The workspace of both entries: rb is the
// ray batch evd_nerf_render packs, z0 the first pass's z
struct NerfRenderWs { float *rb, *z2, *z0, *raw, *wts, *wts0, *zs; };
static const size_t NERF_RENDER_WS_SLACK = 256;     // alignment slack for an unaligned caller pointer
static size_t nerf_render_layout(const evd_render_cfg* cfg, long R, void* workspace, NerfRenderWs* L) {
    const size_t S = cfg->N_samples, Ni = cfg->N_importance > 0 ? cfg->N_importance : 0, St = S + Ni, r = (size_t)R;
    Workspace ws(workspace);
    L->rb = ws.take<float>(r * 11);
    L->z2 = ws.take<float>(r * St);             // z (merged)
    L->z0 = ws.take<float>(r * S); L->raw = ws.take<float>(r * St * 4);
    L->wts = ws.take<float>(r * St); L->wts0 = ws.take<float>(r * S);
    L->zs = ws.take<float>(r * (Ni ? Ni : 1));  // z_samples
    return ws.used() + NERF_RENDER_WS_SLACK;
}
size_t evd_nerf_render_workspace_bytes(const evd_render_cfg* cfg, long R) { NerfRenderWs L; return (!cfg || R < 0) ? 0 : nerf_render_layout(cfg, R, nullptr, &L); }

}  // extern "C"
// where the first pass's z lives: an output the caller asked for, else the workspace slot
static float* render_zc(const evd_render_cfg* cfg, const evd_render_out* out, const NerfRenderWs& L) {
    return cfg->N_importance > 0 ? (out->z_vals0 ? out->z_vals0 : L.z0) : (out->z_vals ? out->z_vals : L.z0);
}
static int render_rays_impl(const evd_nerf* coarse, const evd_nerf* fine, const evd_render_cfg* cfg, const float* rb,
                            long R, const float* t_rand, const float* u, const float* noise0, const float* noise1,
                            evd_render_out* out, void* workspace, size_t workspace_bytes, void* stream, bool z_done) {
    EVD_REQUIRE(coarse && cfg && out && (rb || R == 0), "evd_nerf_render_rays: null argument");
    EVD_REQUIRE((cfg->use_viewdirs != 0) == (coarse->no_views == 0) && (!fine || fine->no_views == coarse->no_views),
                "evd_nerf_render_rays: cfg->use_viewdirs does not match the networks (view branch vs output_linear)");
    const int nc = cfg->use_viewdirs ? 11 : 8;
    EVD_REQUIRE(cfg->N_samples >= 1, "evd_nerf_render_rays: N_samples must be >= 1");
    EVD_REQUIRE(cfg->N_importance <= 0 || fine, "evd_nerf_render_rays: N_importance > 0 needs the fine network");
    EVD_REQUIRE(cfg->N_importance <= 0 || cfg->N_samples >= 3, "evd_nerf_render_rays: hierarchical sampling needs N_samples >= 3");
    EVD_REQUIRE(!(cfg->perturb > 0.f) || (t_rand && (cfg->N_importance <= 0 || u)),
                "evd_nerf_render_rays: perturb > 0 needs explicit t_rand (and u) draws");
    if (R == 0) return EVD_OK;
    NerfRenderWs L;
    const size_t need = nerf_render_layout(cfg, R, workspace, &L);
    if (!workspace || workspace_bytes < need)
        return fail(EVD_E_WORKSPACE, "evd_nerf_render_rays: workspace %zu < %zu bytes", workspace_bytes, need);
    const int S = cfg->N_samples, Ni = cfg->N_importance > 0 ? cfg->N_importance : 0, St = S + Ni;
    float *z2 = L.z2, *raw = L.raw, *wts = L.wts, *wts0 = L.wts0, *zs = L.zs;
    int rc;
    float* zc = render_zc(cfg, out, L);
    if (!z_done && (rc = evd_sample_z(cfg, rb, nc, R, t_rand, zc, stream))) return rc;
    auto pass = [&](const evd_nerf* net, const float* z, int Sp, const float* noise, float* rgb, float* depth, float* acc,
                    float* weights, float* raw_out, float* feat) -> int {
        int rc2 = evd_nerf_mlp(net, cfg->precision, rb, z, R, Sp, raw_out, feat, out->feature_kind ? out->feature_kind : 1, stream);
        if (rc2) return rc2;
        const float thr = (!cfg->is_train && net->rmnear > 0.f) ? (float)((double)net->rmnear / 128.0) : 0.f;
        return evd_raw2outputs(raw_out, z, rb + 3, nc, R, Sp, 4, 3, 0, 3, net->rgb_act, net->sigma_act, cfg->white_bkgd, thr,
                               noise, rgb, nullptr, acc, weights, depth, nullptr, 0, nullptr, stream);
    };
    if (!Ni) {
        float* wo = out->weights ? out->weights : wts;
        float* ro = out->raw ? out->raw : raw;
        return pass(coarse, zc, S, noise0, out->rgb, out->depth, out->acc, wo, ro, out->feature);
    }
    float* w0 = out->weights0 ? out->weights0 : wts0;
    if ((rc = pass(coarse, zc, S, noise0, out->rgb0, out->depth0, out->acc0, w0, raw, nullptr))) return rc;
    float* zm = out->z_vals ? out->z_vals : z2;
    if ((rc = evd_sample_pdf_merge(zc, w0, R, S, Ni, cfg->perturb == 0.f, u, zs, zm, nullptr, out->z_std, stream))) return rc;
    float* wo = out->weights ? out->weights : wts;
    float* ro = out->raw ? out->raw : raw;
    return pass(fine, zm, St, noise1, out->rgb, out->depth, out->acc, wo, ro, out->feature);
}

extern "C" {
int evd_nerf_render_rays(const evd_nerf* coarse, const evd_nerf* fine, const evd_render_cfg* cfg, const float* rb,
                         long R, const float* t_rand, const float* u, const float* noise0, const float* noise1,
                         evd_render_out* out, void* workspace, size_t workspace_bytes, void* stream) {
    return render_rays_impl(coarse, fine, cfg, rb, R, t_rand, u, noise0, noise1, out, workspace, workspace_bytes, stream, false);
}

int evd_nerf_render(const evd_nerf* coarse, const evd_nerf* fine, const evd_render_cfg* cfg, const float* rays, long R,
                    const float* t_rand, const float* u, const float* noise0, const float* noise1,
                    evd_render_out* out, void* workspace, size_t workspace_bytes, void* stream) {
    EVD_REQUIRE(cfg && out && (rays || R == 0), "evd_nerf_render: null argument");
    if (R == 0) return EVD_OK;
    NerfRenderWs L;
    const size_t need = nerf_render_layout(cfg, R, workspace, &L);
    if (!workspace || workspace_bytes < need)
        return fail(EVD_E_WORKSPACE, "evd_nerf_render: workspace %zu < %zu bytes", workspace_bytes, need);
    // ray packing and z stratification in ONE launch (they are 44 B per ray and 4 B per sample)
    const bool fused_z = cfg->use_viewdirs && cfg->N_samples >= 1;
    int rc = fused_z ? evd_ray_batch_z(cfg, rays, R, t_rand, L.rb, render_zc(cfg, out, L), stream) : evd_ray_batch(cfg, rays, R, L.rb, stream);
    if (rc) return rc;
    return render_rays_impl(coarse, fine, cfg, L.rb, R, t_rand, u, noise0, noise1, out, workspace, workspace_bytes, stream, fused_z);
}

}  // extern "C"
