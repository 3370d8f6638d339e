// C-ABI entry points of the PDRF backbone and the mode='c2f' renderer (reference networks/pdrf/voxnerf.py,
// networks/renderer.py:182-217).
#include "evd_common.h"
#include "nerf_mlp.h"
#include "pack.h"
#include "voxel.h"
#include "voxel_generic.h"
#include "nerf_train_generic.h"
#include "voxel_mlp_kernel.h"
#include "voxel_train.h"
#include "awp_embed.h"

#include <cmath>
#include <cstdint>
#include <cstdlib>

// the PDRF level networks keep packed streams for the first four arithmetic modes; EVD_PREC_F16C (compensated float16) has its own
// stream (pipe_c) on the standard fine level; every other level runs EVD_PREC_F16X3 next to it
#define EVD_VOX_NUM_PREC EVD_PREC_F16C

using namespace evd;

struct evd_voxel {
    int num_layers, hidden_dim, geo, num_layers_color, input_ch, ft_dim, app_dim;
    int n_comp[3], grid[3], app_act, rgb_act, sigma_act, composite_feature;
    float aabb[6], rmnear;
    int multires = PE_L, multires_views = PE_LV;
    DevBuf plane[3], line[3], plane_h[3], line_h[3], basis, bias, bias_src, tv_acc, wmaps;
    // fwd: the level's network in the layer table of voxel_mlp_kernel.h, ONE stream per mode of a standard level (is_train_prec): the
    // render pass and the training forward both read it.  stream: the generic kernel's layout (kernel_voxel.hip), built only where
    // voxel_level_forward can select it (has_generic_stream).  bwd: the W^T streams of the training backward.
    PackedStream stream[EVD_VOX_NUM_PREC], fwd[EVD_VOX_NUM_PREC], bwd[EVD_VOX_NUM_PREC][VBWD_NSTREAMS];
    int nchunks[EVD_VOX_NUM_PREC], fwd_chunks[EVD_VOX_NUM_PREC];
    mutable PackedStreamC pipe_c; // compensated float16 mode (voxel_mlp_c_kernel.h): float16 + fp6 fragments and row scales; fine level only
    int pipe_c_chunks = 0;
    // its re-pack after evd_voxel_load_params is LAZY (a training loop re-loads every iteration and never renders in this mode): the new
    // parameter values are kept in `arena_dev` (one stream-ordered device copy) and re-packed by the first f16c launch that follows
    mutable DevBuf arena_dev;
    mutable bool pipe_c_stale = false;
    DevBuf cnet;                  // composite_feature levels: color_net.{0,1,2}.{weight,bias} as float32 in the reference layouts (k_color_rows)
    // sigma_net.0 .. num_layers-1, then color_net.l.{weight,bias} in the parameter arena, [nblk] = total (a standard level: 8 blocks)
    long param_off[VG_MAX_LAYERS + 2 * VG_MAX_LAYERS + 1];
    int nblk;
    // a level of any other shape than the two standard ones (voxel_generic.h): `stream` holds the layout of kernel_voxel_generic.hip in every
    // mode, fwd / bwd / pipe_c stay empty; params_f32 is the float32 copy of the parameters its training backward reads in place
    bool generic = false;
    DevBuf params_f32;
    int sigma_blk(int l) const { return l; }
    int color_w_blk(int l) const { return num_layers + 2 * l; }
    int color_b_blk(int l) const { return num_layers + 2 * l + 1; }
    GridParams gp;
    RepackBatch batch;            // table of every fragment stream, for the one-launch re-pack of evd_voxel_load_params
    mutable SideStream side;      // backward entry: wgrad side stream of THIS handle (created on first use)
};

static const int kMat0[3] = {0, 0, 1}, kMat1[3] = {1, 2, 2}, kVec[3] = {2, 1, 0};

// Where voxel_level_forward can take k_voxel_mlp on a STANDARD level, i.e. which levels and modes need its `stream`: a mode or an encoding
// without a pipelined stream (EVD_PREC_F32, non-standard multires / multires_views), and the standard coarse level (64/15/32) in every mode:
// for per-sample feature rows (also the geo rows of a composite_feature level) it has no other kernel.  The standard fine level's pipelined
// kernels write those rows themselves.
static bool std_coarse(const evd_voxel* v) { return !v->generic && v->hidden_dim == 64; }
static bool has_generic_stream(bool piped, bool coarse) { return !piped || coarse; }

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

// (the float16 copy of one grid value, as evd_voxel_create and k_load_grids make it, is f16_sat of evd_common.h)

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
    int rc = EVD_OK;
    // planes/lines: [1,C,H,W] -> channel-last [H][W][C]
    for (int i = 0; i < 3 && !rc; ++i) {
        v->n_comp[i] = d->n_comp[i]; v->grid[i] = d->grid[i];
        const int C = d->n_comp[i], Wp = d->grid[kMat0[i]], Hp = d->grid[kMat1[i]], Lp = d->grid[kVec[i]];
        std::vector<float> cl((size_t)C * Hp * Wp);
        for (int c = 0; c < C; ++c)
            for (long hw = 0; hw < (long)Hp * Wp; ++hw) cl[(size_t)hw * C + c] = d->plane[i][(size_t)c * Hp * Wp + hw];
        rc = v->plane[i].upload(cl.data(), cl.size() * sizeof(float));
        if (rc) break;
        {   // float16 copy for the half-precision arithmetic modes
            std::vector<_Float16> ch(cl.size());
            for (size_t k = 0; k < cl.size(); ++k) ch[k] = f16_sat(cl[k]);
            rc = v->plane_h[i].upload(ch.data(), ch.size() * sizeof(_Float16));
            if (rc) break;
        }
        std::vector<float> ll((size_t)C * Lp);
        for (int c = 0; c < C; ++c)
            for (int l = 0; l < Lp; ++l) ll[(size_t)l * C + c] = d->line[i][(size_t)c * Lp + l];
        rc = v->line[i].upload(ll.data(), ll.size() * sizeof(float));
        if (rc) break;
        std::vector<_Float16> lh(ll.size());
        for (size_t k = 0; k < ll.size(); ++k) lh[k] = f16_sat(ll[k]);
        rc = v->line_h[i].upload(lh.data(), lh.size() * sizeof(_Float16));
    }
    if (!rc) rc = v->basis.upload(d->basis, sizeof(float) * (size_t)d->app_dim * ctot);
    if (!rc) rc = v->tv_acc.alloc((size_t)6 * 2 * TV_MAX_BLOCKS * sizeof(double));
    if (rc) { evd_voxel_destroy(v); return rc; }
    GridParams& g = v->gp;
    for (int i = 0; i < 3; ++i) {
        g.plane[i] = (const float*)v->plane[i].p; g.line[i] = (const float*)v->line[i].p;
        g.plane_h[i] = (const _Float16*)v->plane_h[i].p; g.line_h[i] = (const _Float16*)v->line_h[i].p;
        g.n_comp[i] = d->n_comp[i]; g.grid[i] = d->grid[i];
        g.aabb_min[i] = d->aabb[i];
        g.inv[i] = 2.0f / (d->aabb[3 + i] - d->aabb[i]);
    }
    g.basis = (const float*)v->basis.p; g.app_dim = d->app_dim; g.app_act = d->app_act;

    // weight streams (order = kernel_voxel.hip k_voxel_mlp).  The parameters are first copied into one host arena in the
    // canonical order sigma_net.0 .., then color_net.l.{weight,bias} (a standard level: sigma_net.0, sigma_net.1,
    // color_net.{0,1,2}.{weight,bias}); every packed element records its arena index so that evd_voxel_load_params can re-pack on the
    // device (pack.h).  Layer shapes: voxnerf.py:48-82 (the colour network's hidden width is hidden_dim, :73,78).
    const int T = HD / 32, KS = HD / 16, KF = FT / 16;
    const int nblk = v->nblk;
    long psz[VG_MAX_LAYERS + 2 * VG_MAX_LAYERS];
    const float* srcs[VG_MAX_LAYERS + 2 * VG_MAX_LAYERS];
    for (int l = 0; l < NS; ++l) {
        psz[v->sigma_blk(l)] = (long)(l == NS - 1 ? 1 + G : HD) * (l == 0 ? d->input_ch : HD);
        srcs[v->sigma_blk(l)] = d->sigma_w[l];
    }
    for (int l = 0; l < NC; ++l) {
        const long out = l == NC - 1 ? 3 : HD;
        psz[v->color_w_blk(l)] = out * (l == 0 ? G + ICV : HD);
        psz[v->color_b_blk(l)] = out;
        srcs[v->color_w_blk(l)] = d->color_w[l];
        srcs[v->color_b_blk(l)] = d->color_b[l];
    }
    long total = 0;
    for (int i = 0; i < nblk; ++i) { v->param_off[i] = total; total += psz[i]; }
    v->param_off[nblk] = total;
    std::vector<float> arena((size_t)total, 0.f);
    for (int i = 0; i < nblk; ++i)
        if (srcs[i]) memcpy(arena.data() + v->param_off[i], srcs[i], psz[i] * sizeof(float));
    if (v->composite_feature) {       // the colour network runs per RAY on the composited features (voxnerf.py:231-239): plain float32 rows
        rc = v->cnet.upload(arena.data() + v->param_off[NS], (size_t)(v->param_off[nblk] - v->param_off[NS]) * sizeof(float));
        if (rc) { evd_voxel_destroy(v); return rc; }
    }
    const float* A = arena.data();
    // A generic level (voxel_generic.h): the layer table of kernel_voxel_generic.hip in every mode; no pipelined, f16c or training streams
    auto generic_streams = [&]() -> int {
            const int GTg = (G + 31) / 32;
            auto hid_col = [](int j, int kk) { return 16 * j + phi(kk); };
            auto in0_col = [&](int j, int kk) {            // cat([fts, PE(pts)]): VG_KF natural feature k-steps (absent channels: zero), then the PE arrangement
                if (j < VG_KF) return 16 * j + kk < FT ? 16 * j + kk : -1;
                const int c = pe_src_col(L, 8 * (j - VG_KF) + (kk & 7), kk >> 3);
                return c < 0 ? -1 : FT + c;
            };
            auto c0_col = [&](int j, int kk) {             // cat([h[..., 1:], PE(dirs)]) voxnerf.py:248: VG_GK geo k-steps, then the PE arrangement
                if (j < VG_GK) { const int c = 16 * j + phi(kk); return c < G ? c : -1; }
                const int c = pe_src_col(Lv, 8 * (j - VG_GK) + (kk & 7), kk >> 3);
                return c < 0 ? -1 : G + c;
            };
            auto W_sig = [&](int l) { return A + v->param_off[v->sigma_blk(l)]; };
            auto W_col = [&](int l) { return A + v->param_off[v->color_w_blk(l)]; };
            auto build_generic = [&](StreamBuilder& sb) {
                for (int l = 0; l + 1 < NS; ++l) {
                    if (l == 0) sb.layer(W_sig(0), HD, d->input_ch, T, VG_KF + PE_KS, true, in0_col);
                    else sb.layer(W_sig(l), HD, HD, T, KS, true, hid_col);
                }
                {   // the last sigma layer: the density row, then the geo rows in 32-channel tiles
                    const float* Wl = W_sig(NS - 1);
                    const int in_dim = NS == 1 ? d->input_ch : HD, ks = NS == 1 ? VG_KF + PE_KS : KS;
                    auto sig_row = [](int, int r) { return r == 0 ? 0 : -1; };
                    if (NS == 1) sb.layer_rc(Wl, in_dim, 1, ks, true, sig_row, in0_col);
                    else sb.layer_rc(Wl, in_dim, 1, ks, true, sig_row, hid_col);
                    for (int t = 0; t < GTg; ++t) {
                        auto geo_row = [G, t](int, int r) { return 32 * t + r < G ? 1 + 32 * t + r : -1; };
                        if (NS == 1) sb.layer_rc(Wl, in_dim, 1, ks, true, geo_row, in0_col);
                        else sb.layer_rc(Wl, in_dim, 1, ks, true, geo_row, hid_col);
                    }
                }
                for (int l = 0; l < NC; ++l) {
                    const int out = l == NC - 1 ? 3 : HD, tiles = l == NC - 1 ? 1 : T;
                    if (l == 0) sb.layer(W_col(0), out, G + ICV, tiles, VG_GK + PEV_KS, true, c0_col);
                    else sb.layer(W_col(l), out, HD, tiles, KS, true, hid_col);
                }
            };
            for (int prec = 0; prec < EVD_VOX_NUM_PREC; ++prec) {
                v->nchunks[prec] = v->fwd_chunks[prec] = 0;
                StreamBuilder sb(prec);
                sb.arena = A;
                build_generic(sb);
                v->nchunks[prec] = (int)(sb.bytes.size() / chunk_bytes(prec));
                if ((rc = v->stream[prec].upload(sb))) return rc;
            }
        return v->params_f32.upload(A, (size_t)total * sizeof(float));
    };
    // A standard level: the streams of k_voxel_mlp, of the pipelined / resident / f16c kernels and of the training backward, and the wgrad index maps
    auto standard_streams = [&]() -> int {
        const float *sigma_w0 = A + v->param_off[0], *sigma_w1 = A + v->param_off[1], *color_w0 = A + v->param_off[2], *color_w1 = A + v->param_off[4],
                    *color_w2 = A + v->param_off[6];
        const bool small = (1 + G) <= 32;
        const int GT = (G + 31) / 32, GK = 2 * GT;
        auto hid_col = [](int j, int kk) { return 16 * j + phi(kk); };
        auto in0_col = [&](int j, int kk) {            // cat([fts, PE(pts)]): natural feature k-steps then the PE arrangement
            if (j < KF) return 16 * j + kk;
            const int c = pe_src_col(L, 8 * (j - KF) + (kk & 7), kk >> 3);
            return c < 0 ? -1 : FT + c;
        };
        auto c0_col = [&](int j, int kk) {             // cat([h[...,1:], PE(dirs)]) voxnerf.py:248
            const int gk = small ? 1 : G / 16;
            if (j < gk) {
                const int row = 16 * j + phi(kk);      // index into the sigma-layer output tile(s)
                return small ? (row >= 1 && row <= G ? row - 1 : -1) : row;
            }
            const int c = pe_src_col(Lv, 8 * (j - gk) + (kk & 7), kk >> 3);
            return c < 0 ? -1 : G + c;
        };
        auto build = [&](StreamBuilder& sb) {
            sb.layer(sigma_w0, HD, d->input_ch, T, KF + PE_KS, false, in0_col);
            if (small) {
                sb.layer(sigma_w1, 1 + G, HD, 1, KS, false, hid_col);
            } else {
                sb.layer_rc(sigma_w1, HD, 1, KS, false, [](int, int r) { return r == 0 ? 0 : -1; }, hid_col);       // sigma row
                sb.layer_rc(sigma_w1, HD, G / 32, KS, false, [](int t, int r) { return 1 + 32 * t + r; }, hid_col); // geo rows
            }
            sb.layer(color_w0, HD, G + ICV, T, (small ? 1 : G / 16) + PEV_KS, false, c0_col);
            sb.layer(color_w1, HD, HD, T, KS, false, hid_col);
            sb.layer(color_w2, 3, HD, 1, KS, true, hid_col);
        };
        // the same network in the layer table of voxel_mlp_kernel.h VoxNet (any level): sigma and geo always separate layers, the
        // geo channels in GT zero-padded tiles
        auto build_pipe = [&](StreamBuilder& sb) {
            auto c0p = [&](int j, int kk) {
                if (j < GK) { const int c = 16 * j + phi(kk); return c < G ? c : -1; }
                const int c = pe_src_col(Lv, 8 * (j - GK) + (kk & 7), kk >> 3);
                return c < 0 ? -1 : G + c;
            };
            sb.layer(sigma_w0, HD, d->input_ch, T, KF + PE_KS, false, in0_col);
            sb.layer_rc(sigma_w1, HD, 1, KS, false, [](int, int r) { return r == 0 ? 0 : -1; }, hid_col);
            sb.layer_rc(sigma_w1, HD, GT, KS, false, [G](int t, int r) { return 32 * t + r < G ? 1 + 32 * t + r : -1; }, hid_col);
            sb.layer(color_w0, HD, G + ICV, T, GK + PEV_KS, false, c0p);
            sb.layer(color_w1, HD, HD, T, KS, false, hid_col);
            sb.layer(color_w2, 3, HD, 1, KS, true, hid_col);
        };
        for (int prec = 0; prec < EVD_VOX_NUM_PREC; ++prec) {
            const bool piped = standard && is_train_prec(prec);
            v->nchunks[prec] = v->fwd_chunks[prec] = 0;
            if (has_generic_stream(piped, std_coarse(v))) {
                StreamBuilder sb(prec);
                sb.arena = A;
                build(sb);
                v->nchunks[prec] = (int)(sb.bytes.size() / chunk_bytes(prec));
                if ((rc = v->stream[prec].upload(sb))) return rc;
            }
            if (!piped) continue;
            {   // same layers, single-tile groups, 16 KiB chunks (voxel_mlp_kernel.h): render and training forward
                StreamBuilder sp(prec, PIPE_CB);
                sp.arena = A;
                sp.group = 1;
                build_pipe(sp);
                v->fwd_chunks[prec] = (int)(sp.bytes.size() / PIPE_CB);
                if ((rc = v->fwd[prec].upload(sp))) return rc;
            }
            // the W^T streams of the dgrad chain (voxel_train_kernel.h)
            auto put = [&](int which, auto fill) {
                StreamBuilder sb2(prec, PIPE_CB);
                sb2.arena = A;
                sb2.group = 1;
                fill(sb2);
                return v->bwd[prec][which].upload(sb2);
            };
            rc = put(VBWD_C2, [&](StreamBuilder& b) { b.layer_transposed(color_w2, 3, HD, 0, HD, nullptr, 0, T, 1, true, [](int, int kk) { return kk < 3 ? kk : -1; }); });
            if (!rc) rc = put(VBWD_C1, [&](StreamBuilder& b) { b.layer_transposed(color_w1, HD, HD, 0, HD, nullptr, 0, T, KS, true, hid_col); });
            // rows of an encoding appended to a W^T layer: output row idx of the extra tiles <-> encoding column, so that the output
            // fragments come out in the encoding's own arrangement (fragment j, position kk <-> pe_src_col(L, 8 j + (kk & 7), kk >> 3))
            auto enc_row = [](int L_, int idx) { const int j = idx / 16, kk = phi_inv(idx % 16); return pe_src_col(L_, 8 * j + (kk & 7), kk >> 3); };
            if (!rc) rc = put(VBWD_C0, [&](StreamBuilder& b) {       // [geo rows | direction-encoding rows] of color_net.0
                b.layer_at(GT + 1, KS, true,
                           [&](int t, int r) { if (t < GT) return 32 * t + r < G ? 32 * t + r : -1; const int c = enc_row(Lv, r); return c < 0 ? -1 : G + c; },
                           hid_col, [&](int r, int c) { return color_w0 + (size_t)c * (G + ICV) + r; });
            });
            if (!rc) rc = put(VBWD_SIGGEO, [&](StreamBuilder& b) {
                b.layer_transposed(sigma_w1, 1 + G, HD, 0, HD, nullptr, 0, T, GK + 1, true, [&](int j, int kk) {
                    if (j < GK) { const int c = 16 * j + phi(kk); return c < G ? 1 + c : -1; }
                    return kk == 0 ? 0 : -1;
                });
            });
            if (!rc) rc = put(VBWD_L0, [&](StreamBuilder& b) {       // [feature rows | point-encoding rows] of sigma_net.0
                const int FTT = (FT + 31) / 32, in_dim = d->input_ch;
                b.layer_at(FTT + 2, KS, true,
                           [&](int t, int r) { if (t < FTT) return 32 * t + r < FT ? 32 * t + r : -1; const int c = enc_row(L, 32 * (t - FTT) + r); return c < 0 ? -1 : FT + c; },
                           hid_col, [&](int r, int c) { return sigma_w0 + (size_t)c * in_dim + r; });
            });
            if (rc) return rc;
        }
        if (standard && voxel_mlp_c_chunks(HD, G, FT) > 0) {     // compensated float16 mode: the layer table of voxel_mlp_c_kernel.h VoxNetC (groups of two tiles, 64-input blocks)
            auto c0p = [&](int j, int kk) {
                if (j < GK) { const int c = c_hid_col(j, kk); return c < G ? c : -1; }
                const int c = pe_src_col(Lv, 8 * (j - GK) + (kk & 7), kk >> 3);
                return c < 0 ? -1 : G + c;
            };
            auto sig_at = [=](int r, int c) -> const float* { return c < HD ? sigma_w1 + (size_t)r * HD + c : nullptr; };
            StreamBuilderC sc(PIPE_CB);
            sc.arena = A;
            sc.layer(sigma_w0, HD, d->input_ch, T, KF + PE_KS, 2, in0_col);
            sc.layer_at(1, KS, 1, [](int, int r) { return r == 0 ? 0 : -1; }, c_hid_col, sig_at);
            sc.layer_at(GT, KS, 2, [G](int t, int r) { return 32 * t + r < G ? 1 + 32 * t + r : -1; }, c_hid_col, sig_at);
            sc.layer(color_w0, HD, G + ICV, T, GK + PEV_KS, 2, c0p);
            sc.layer(color_w1, HD, HD, T, KS, 2, c_hid_col);
            sc.layer(color_w2, 3, HD, 1, KS, 1, c_hid_col);
            v->pipe_c_chunks = (int)(sc.bytes.size() / PIPE_CB);
            if (v->pipe_c_chunks != voxel_mlp_c_chunks(HD, G, FT))
                rc = fail(EVD_E_INVALID, "evd_voxel_create: f16c stream has %d chunks, kernel expects %d", v->pipe_c_chunks, voxel_mlp_c_chunks(HD, G, FT));
            if (!rc) rc = v->pipe_c.upload(sc);
            if (rc) return rc;
        }
        {   // wgrad index maps (voxel_train.h)
            std::vector<int> m(VMAP_TOTAL, -1);
            for (int i = 0; i < 256; ++i) { const int c = hid_col(i / 16, i % 16); m[VMAP_HID + i] = c < HD ? c : -1; }
            for (int i = 0; i < 64; ++i) {
                m[VMAP_FTS + i] = i < FT ? i : -1;
                const int c = pe_src_col(L, 8 * (i / 16) + (i % 16 & 7), (i % 16) >> 3);
                m[VMAP_PE + i] = c < 0 ? -1 : FT + c;
            }
            for (int i = 0; i < 32; ++i) {
                const int c = pe_src_col(Lv, 8 * (i / 16) + (i % 16 & 7), (i % 16) >> 3);
                m[VMAP_DIR + i] = c < 0 ? -1 : G + c;
            }
            for (int i = 0; i < 128; ++i) {
                const int c = hid_col(i / 16, i % 16);
                m[VMAP_GEO_X + i] = c < G ? c : -1;
                m[VMAP_GEO_Y + i] = c < G ? 1 + c : -1;
            }
            for (int i = 0; i < 3; ++i) m[VMAP_COL + i] = i;
            m[VMAP_SIG] = 0;
            for (int i = 0; i < 16; ++i) { m[VMAP_F64_SG + i] = m[VMAP_GEO_Y + i]; m[VMAP_F64_SG + 16 + i] = m[VMAP_SIG + i]; }
            for (int i = 0; i < 32; ++i) { m[VMAP_F64_C0 + i] = m[VMAP_GEO_X + i]; m[VMAP_F64_C0 + 32 + i] = m[VMAP_DIR + i]; }
            for (int i = 0; i < 32; ++i) m[VMAP_F64_L0 + i] = m[VMAP_FTS + i];
            for (int i = 0; i < 64; ++i) m[VMAP_F64_L0 + 32 + i] = m[VMAP_PE + i];
            for (int i = 0; i < 128; ++i) m[VMAP_SG5 + i] = m[VMAP_GEO_Y + i];
            for (int i = 0; i < 32; ++i) m[VMAP_SG5 + 128 + i] = m[VMAP_SIG + i];
            if ((rc = v->wmaps.upload(m.data(), m.size() * sizeof(int)))) return rc;
        }
        return EVD_OK;
    };
    if ((rc = generic ? generic_streams() : standard_streams())) { evd_voxel_destroy(v); return rc; }
    std::vector<float> b(32 * 16, 0.f);            // zero block shared by the bias-free sigma layers
    std::vector<int32_t> bsrc(32 * 16, -1);
    auto push = [&](int block, int out_dim, int tiles) {
        for (int i = 0; i < tiles * 32; ++i) {
            b.push_back(i < out_dim ? A[v->param_off[block] + i] : 0.f);
            bsrc.push_back(i < out_dim ? (int32_t)(v->param_off[block] + i) : -1);
        }
    };
    for (int l = 0; l < NC; ++l) push(v->color_b_blk(l), l == NC - 1 ? 3 : HD, l == NC - 1 ? 1 : T);
    rc = v->bias.upload(b.data(), b.size() * sizeof(float));
    if (!rc) rc = v->bias_src.upload(bsrc.data(), bsrc.size() * sizeof(int32_t));
    if (rc) { evd_voxel_destroy(v); return rc; }
    *out = v;
    return EVD_OK;
}

int evd_voxel_sample(const evd_voxel* v, const float* pts, long n, float* out, int out_stride, int out_col, void* stream) {
    EVD_REQUIRE(v && out && n >= 0 && out_stride >= out_col + v->app_dim, "evd_voxel_sample: bad arguments");
    if (n == 0) return EVD_OK;
    return launch_voxel_sample(v->gp, false, pts, n, out, out_stride, out_col, as_stream(stream));
}

// sampling inside the c2f render: the half-precision arithmetic modes read the float16 copies of the grids
static bool grids_half_for(const evd_voxel* v, int precision) {
    if (precision == EVD_PREC_BF16 || precision == EVD_PREC_F16) return true;
    // The compensated mode: the level that is FED by the previous one (its features are cat([previous level's, its own]) -- the fine
    // level of a c2f render, whose output is the image) reads the float16 copies of its grids: their 2^-12 rounding is random over 96
    // channels and six taps and costs nothing measurable (trained blurfactory-size model: RGB L-inf 8.4e-6 against 7.9e-6 on the
    // float32 grids, bound 1e-4), and the gather moves half the bytes (c2f render 0.708 -> 0.683 ms).  The coarse level keeps the
    // float32 grids: its weights place the importance samples, and with float16 grids there the FINE image is at 1.0e-4.
    // The coarse features AT THE IMPORTANCE SAMPLES (renderer.py:209) also feed the fine networks only -- but there the float16 grids
    // cost 3.4e-5 of the fine image for ~1 % of the render: left on the float32 grids.
    // A generic level has no compensated kernel: EVD_PREC_F16C is EVD_PREC_F16X3 there, grids included (as on the standard coarse level)
    if (precision == EVD_PREC_F16C) return !v->generic && v->ft_dim > v->app_dim;
    return false;
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

// colour network of a composite_feature level, per RAY (voxnerf.py:231-239): h = cat([feature_map, PE(dirs)]) -> Linear + ReLU
// (num_layers_color - 1 times) -> Linear -> sigmoid.  A wavefront per ray, a lane per hidden unit (HD <= 256: up to 4 units per lane);
// the weights are the reference's float32 [out, in] rows, read through the caches (7 k MACs per ray: nothing to optimise).
static __global__ __launch_bounds__(256) void k_color_rows(const float* __restrict__ cnet, const float* __restrict__ fm, const float* __restrict__ viewdirs,
                                                           int vd_stride, long R, int G, int HD, int Lv, float* __restrict__ color) {
    __shared__ float in[4][160], h0[4][256], h1[4][256];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + w;
    const int icv = 3 * (1 + 2 * Lv), nin = G + icv;
    const float *w0 = cnet, *b0 = w0 + (long)HD * nin, *w1 = b0 + HD, *b1 = w1 + (long)HD * HD, *w2 = b1 + HD, *b2 = w2 + 3L * HD;
    if (r < R) {
        for (int i = lane; i < nin; i += 64) {
            float x;
            if (i < G) x = fm[r * G + i];
            else {
                const int c = i - G;              // embedding.py:88-98: [x, sin(x f0), cos(x f0), sin(x f1), ...], 3 values each
                const float d = viewdirs[r * vd_stride + c % 3];
                x = c < 3 ? d : ((c - 3) / 3 % 2 == 0 ? sinf(d * (float)(1 << ((c - 3) / 6))) : cosf(d * (float)(1 << ((c - 3) / 6))));
            }
            in[w][i] = x;
        }
    }
    __syncthreads();
    if (r < R)
        for (int j = lane; j < HD; j += 64) {
            float s = b0[j];
            for (int i = 0; i < nin; ++i) s = fmaf(w0[(long)j * nin + i], in[w][i], s);
            h0[w][j] = fmaxf(s, 0.f);
        }
    __syncthreads();
    if (r < R)
        for (int j = lane; j < HD; j += 64) {
            float s = b1[j];
            for (int i = 0; i < HD; ++i) s = fmaf(w1[(long)j * HD + i], h0[w][i], s);
            h1[w][j] = fmaxf(s, 0.f);
        }
    __syncthreads();
    if (r < R && lane < 3) {
        float s = b2[lane];
        for (int i = 0; i < HD; ++i) s = fmaf(w2[(long)lane * HD + i], h1[w][i], s);
        color[r * 3 + lane] = 1.f / (1.f + expf(-s));            // torch.sigmoid(h) voxnerf.py:239
    }
}

// what the inference pass and the training forward of a level fill alike (the stream is chosen later, with the kernel)
static VoxMlpParams vox_mlp_params(const evd_voxel* v, const float* pts, const float* viewdirs, int vd_stride, const float* fts, int ft_stride,
                                   long R, int S, float* raw, float* feature, char* act) {
    VoxMlpParams p{};
    p.pts = pts; p.viewdirs = viewdirs; p.fts = fts; p.nsamp = R * (long)S; p.S = S; p.vd_stride = vd_stride; p.ft_stride = ft_stride;
    p.bias = (const float*)v->bias.p; p.nbias = (int)(v->bias.bytes / sizeof(float)); p.raw = raw; p.feature = feature; p.act = act;
    return p;
}

// the compensated mode's stream into p, re-packed first if evd_voxel_load_params has run since its last use
static int use_pipe_c(const evd_voxel* v, VoxMlpParams& p, hipStream_t st) {
    if (v->pipe_c_stale) {
        int rc = repack_stream_c(v->pipe_c, (const float*)v->arena_dev.p, st);
        if (rc) return rc;
        v->pipe_c_stale = false;
    }
    p.wstream = (const char*)v->pipe_c.data.p;
    p.wscale = (const unsigned*)v->pipe_c.scales.p;
    p.nchunks = v->pipe_c_chunks;
    return EVD_OK;
}

// The network of a level's inference pass: picks the kernel and, with it, the stream of the handle it reads (p.wstream / p.nchunks).
static int voxel_level_forward(const evd_voxel* v, int precision, VoxMlpParams& p, hipStream_t st) {
    if (v->generic) {       // any other shape: its own kernel and stream in every mode; EVD_PREC_F16C runs float32-grade as on the standard coarse level
        const int prec = precision == EVD_PREC_F16C ? EVD_PREC_F16X3 : precision;
        p.wstream = (const char*)v->stream[prec].data.p;
        p.nchunks = v->nchunks[prec];
        const VoxGenShape g{v->num_layers, v->num_layers_color, v->geo, (v->geo + 31) / 32, v->ft_dim / 16};
        return voxel_mlp_generic_dispatch(prec, v->hidden_dim, p, g, st);
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
        hipLaunchKernelGGL(k_color_rows, dim3((unsigned)cdiv(R, 4L)), dim3(256), 0, st, (const float*)v->cnet.p, cmap, viewdirs, vd_stride, R, v->geo,
                           v->hidden_dim, v->multires_views, color);
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

// ---- training: the level's sigma / colour networks -----------------------------------------------------
static const int VOX_WGRAD_BLOCKS = 256;
static long vox_tiles(long nsamp) { return cdiv(nsamp, 256L) * 8; }
// EVD_PREC_F16C trains on the single-product float16 store and backward behind a compensated forward: the level's f16c kernel where
// that is built (fine level), else the split-float16 forward writing the float16 store (coarse level)
// EVD_PREC_F16M: the split-float16 forward on every level, same store and backward
static bool vox_train_built(const evd_voxel* v, int prec) {
    if (v->generic) return prec == EVD_PREC_F16X3;      // kernel_voxel_train_generic.hip; the other modes' training kernels are the standard levels'
    if (prec == EVD_PREC_F16C) return v->fwd_chunks[EVD_PREC_F16] > 0 && (v->pipe_c_chunks > 0 || v->fwd_chunks[EVD_PREC_F16X3] > 0);
    if (prec == EVD_PREC_F16M) return v->fwd_chunks[EVD_PREC_F16] > 0 && v->fwd_chunks[EVD_PREC_F16X3] > 0;
    return prec >= 0 && prec < EVD_VOX_NUM_PREC && v->fwd_chunks[prec] > 0;
}
static int vox_store_prec(int prec) { return (prec == EVD_PREC_F16C || prec == EVD_PREC_F16M) ? EVD_PREC_F16 : prec; }

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
    EVD_REQUIRE(!v->composite_feature, "evd_voxel_mlp_train: composite_feature levels (kernel_type PBE) are built for inference only");
    EVD_REQUIRE(!v->generic || precision == EVD_PREC_F16X3, "evd_voxel_mlp_train: a level of this shape (hidden %d, geo %d, features %d, %d + %d layers) "
                "trains in precision f16x3 only; the other training modes are built for the standard levels (64/15/32 and 256/128/64 with 2 + 3 layers)",
                v->hidden_dim, v->geo, v->ft_dim, v->num_layers, v->num_layers_color);
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
        const VoxGenShape g{v->num_layers, v->num_layers_color, v->geo, (v->geo + 31) / 32, v->ft_dim / 16};
        return voxel_train_fwd_generic_dispatch(v->hidden_dim, p, g, as_stream(stream));
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

int evd_voxel_geo_feat_dim(const evd_voxel* v) { return v ? v->geo : 0; }

int evd_voxel_mlp_backward(const evd_voxel* v, int precision, const float* d_raw, const float* raw, const float* d_feature, const void* awp_store,
                           size_t awp_store_bytes, long R, int S, void* store,
                           size_t store_bytes, const evd_voxel_grads* grads, float* d_fts, int d_fts_stride, const float* pts, const float* viewdirs, int vd_stride,
                           float* d_pts, float* d_dirs, void* workspace, size_t workspace_bytes, void* stream) {
    EVD_REQUIRE((!d_pts || pts) && (!d_dirs || viewdirs), "evd_voxel_mlp_backward: d_pts / d_dirs need the forward's pts / viewdirs");
    EVD_REQUIRE(v && d_raw && raw && store && grads && workspace, "evd_voxel_mlp_backward: null argument");
    EVD_REQUIRE(!v->generic || precision == EVD_PREC_F16X3, "evd_voxel_mlp_backward: a level of this shape (hidden %d, geo %d, features %d, %d + %d layers) "
                "trains in precision f16x3 only; the other training modes are built for the standard levels (64/15/32 and 256/128/64 with 2 + 3 layers)",
                v->hidden_dim, v->geo, v->ft_dim, v->num_layers, v->num_layers_color);
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

// ---- training: the grids as parameters -------------------------------------------------------------------------------
int evd_voxel_grid_sizes(const evd_voxel* v, long* sizes) {
    EVD_REQUIRE(v && sizes, "evd_voxel_grid_sizes: null argument");
    for (int i = 0; i < 3; ++i) {
        sizes[i] = (long)(v->plane[i].bytes / sizeof(float));
        sizes[3 + i] = (long)(v->line[i].bytes / sizeof(float));
    }
    sizes[6] = (long)(v->basis.bytes / sizeof(float));
    return EVD_OK;
}

int evd_voxel_get_grids(const evd_voxel* v, float* const* plane, float* const* line, float* basis, void* stream) {
    EVD_REQUIRE(v && plane && line && basis, "evd_voxel_get_grids: null argument");
    hipStream_t st = as_stream(stream);
    for (int i = 0; i < 3; ++i) {
        EVD_HIP(hipMemcpyAsync(plane[i], v->plane[i].p, v->plane[i].bytes, hipMemcpyDeviceToDevice, st));
        EVD_HIP(hipMemcpyAsync(line[i], v->line[i].p, v->line[i].bytes, hipMemcpyDeviceToDevice, st));
    }
    EVD_HIP(hipMemcpyAsync(basis, v->basis.p, v->basis.bytes, hipMemcpyDeviceToDevice, st));
    return EVD_OK;
}

// the seven tensors of a level in ONE launch: every source value is read once and written twice, as the float32 copy the float32-grade modes
// and the backward gather, and as the float16 copy the half-precision modes gather (13 launches and a second read of 165 MB before)
struct GridLoadSeg { const float* src; float* dst; _Float16* dst_h; long n4, tail0, n; };
struct GridLoadSegs { GridLoadSeg s[7]; };
static __global__ __launch_bounds__(256) void k_load_grids(const GridLoadSegs segs) {
    const GridLoadSeg s = segs.s[blockIdx.y];
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < s.n4; i += stride) {
        const f32x4 v = reinterpret_cast<const f32x4*>(s.src)[i];
        reinterpret_cast<f32x4*>(s.dst)[i] = v;
        if (s.dst_h) {
            typedef _Float16 h4 __attribute__((ext_vector_type(4)));
            const h4 h = {f16_sat(v[0]), f16_sat(v[1]), f16_sat(v[2]), f16_sat(v[3])};
            reinterpret_cast<h4*>(s.dst_h)[i] = h;
        }
    }
    for (long i = s.tail0 + (long)blockIdx.x * 256 + threadIdx.x; i < s.n; i += stride) {
        s.dst[i] = s.src[i];
        if (s.dst_h) s.dst_h[i] = f16_sat(s.src[i]);
    }
}

int evd_voxel_load_grids(evd_voxel* v, const float* const* plane, const float* const* line, const float* basis, void* stream) {
    EVD_REQUIRE(v && plane && line && basis, "evd_voxel_load_grids: null argument");
    hipStream_t st = as_stream(stream);
    GridLoadSegs segs;
    long nmax = 0;
    auto seg = [&](int k, const float* src, DevBuf& dst, DevBuf* dst_h) {
        const long n = (long)(dst.bytes / sizeof(float));
        const bool vec = ((uintptr_t)src % 16) == 0;            // device allocations are 256-byte aligned; a caller's slice may not be
        segs.s[k] = GridLoadSeg{src, (float*)dst.p, dst_h ? (_Float16*)dst_h->p : nullptr, vec ? n / 4 : 0, vec ? (n / 4) * 4 : 0, n};
        nmax = n > nmax ? n : nmax;
    };
    for (int i = 0; i < 3; ++i) {
        EVD_REQUIRE(plane[i] && line[i], "evd_voxel_load_grids: missing grid %d", i);
        seg(i, plane[i], v->plane[i], &v->plane_h[i]);
        seg(3 + i, line[i], v->line[i], &v->line_h[i]);
    }
    seg(6, basis, v->basis, nullptr);
    const long bx = cdiv(nmax / 4 + 1, 256L) < 2048 ? cdiv(nmax / 4 + 1, 256L) : 2048;
    hipLaunchKernelGGL(k_load_grids, dim3((unsigned)bx, 7), dim3(256), 0, st, segs);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int evd_voxel_grid_mirrors(const evd_voxel* v, float** plane_f32, float** line_f32, float** basis_f32, void** plane_f16, void** line_f16) {
    EVD_REQUIRE(v && plane_f32 && line_f32 && basis_f32 && plane_f16 && line_f16, "evd_voxel_grid_mirrors: null argument");
    for (int i = 0; i < 3; ++i) {
        plane_f32[i] = (float*)v->plane[i].p; line_f32[i] = (float*)v->line[i].p;
        plane_f16[i] = v->plane_h[i].p; line_f16[i] = v->line_h[i].p;
    }
    *basis_f32 = (float*)v->basis.p;
    return EVD_OK;
}

static GridGrads grid_grads(const evd_voxel_grid_grads* g) {
    GridGrads gg;
    for (int i = 0; i < 3; ++i) { gg.plane[i] = g->plane[i]; gg.line[i] = g->line[i]; }
    gg.basis = g->basis;
    return gg;
}

int evd_voxel_sample_bwd(const evd_voxel* v, const float* pts, long n, const float* d_out, int d_stride, int d_col,
                         const evd_voxel_grid_grads* g, float* d_pts, void* stream) {
    EVD_REQUIRE(v && pts && d_out && g && n >= 0 && d_stride >= d_col + v->app_dim, "evd_voxel_sample_bwd: bad arguments");
    EVD_REQUIRE(v->app_act == EVD_ACT_NONE, "evd_voxel_sample_bwd: only app_actfn none is built (all shipped configs)");
    if (n == 0) return EVD_OK;
    const GridGrads gg = grid_grads(g);
    return launch_voxel_sample_bwd(v->gp, pts, n, d_out, d_stride, d_col, gg, d_pts, as_stream(stream));
}

size_t evd_voxel_sample_bwd_workspace_bytes(const evd_voxel* v, long n) {
    if (!v || n <= 0) return 0;
    return voxel_scatter_hybrid_workspace_bytes(v->gp, n);
}

static int sample_bwd_ws(const evd_voxel* v, bool half_grids, const float* pts, long n, const float* d_out, int d_stride, int d_col,
                         const evd_voxel_grid_grads* g, float* d_pts, void* workspace, size_t workspace_bytes, void* stream);
int evd_voxel_sample_bwd_ws(const evd_voxel* v, const float* pts, long n, const float* d_out, int d_stride, int d_col,
                            const evd_voxel_grid_grads* g, float* d_pts, void* workspace, size_t workspace_bytes, void* stream) {
    return sample_bwd_ws(v, false, pts, n, d_out, d_stride, d_col, g, d_pts, workspace, workspace_bytes, stream);
}
int evd_voxel_sample_bwd_prec(const evd_voxel* v, int precision, const float* pts, long n, const float* d_out, int d_stride, int d_col,
                              const evd_voxel_grid_grads* g, float* d_pts, void* workspace, size_t workspace_bytes, void* stream) {
    EVD_REQUIRE(precision >= 0 && precision <= EVD_PREC_F16M, "evd_voxel_sample_bwd_prec: unknown precision %d", precision);
    return sample_bwd_ws(v, v && grids_half_for(v, precision), pts, n, d_out, d_stride, d_col, g, d_pts, workspace, workspace_bytes, stream);
}
static int sample_bwd_ws(const evd_voxel* v, bool half_grids, const float* pts, long n, const float* d_out, int d_stride, int d_col,
                         const evd_voxel_grid_grads* g, float* d_pts, void* workspace, size_t workspace_bytes, void* stream) {
    EVD_REQUIRE(v && pts && d_out && g && n >= 0 && d_stride >= d_col + v->app_dim, "evd_voxel_sample_bwd_ws: bad arguments");
    EVD_REQUIRE(v->app_act == EVD_ACT_NONE, "evd_voxel_sample_bwd_ws: only app_actfn none is built (all shipped configs)");
    if (n == 0) return EVD_OK;
    const GridGrads gg = grid_grads(g);
    if (workspace && workspace_bytes > 0 && voxel_scatter_hybrid_ok(v->gp, n))
        return launch_voxel_sample_bwd_hybrid(v->gp, pts, n, d_out, d_stride, d_col, gg, d_pts, workspace, workspace_bytes, as_stream(stream), half_grids);
    return launch_voxel_sample_bwd(v->gp, pts, n, d_out, d_stride, d_col, gg, d_pts, as_stream(stream));
}

// ---- the deterministic scatter (kernel_voxel_scatter_det.hip; run_nerf.py:50)
// the exponent k of the fixed-point scale 2^k (unit 2^-k): with frexpf(cmax) -> E (cmax < 2^E) and h = ceil(log2(4 n)), k = 62 - h - E; a cell
// receives at most 4 n terms of magnitude < 2^E, so its sum stays below 2^62.  k is clamped to 126 (k_scatter_lines' clamp: 2^k stays a
// finite float32; a batch whose maximum is that small is resolved to 2^-126).  0 where no scale exists (cmax not finite, not positive).
int evd_scatter_det_unit_exp(float cmax, long n) {
    if (!(cmax > 0.f) || !std::isfinite(cmax) || n < 1) return 0;
    int E;
    (void)frexpf(cmax, &E);
    int h = 0;
    while (h < 62 && (1L << h) < 4 * n) ++h;
    const int k = 62 - h - E;
    return k > 126 ? 126 : k;
}

// the region of the workspace behind its 256-byte alignment: the shadow, or (a batch without a scale) the hybrid form's scratch
static size_t det_region_bytes(const evd_voxel* v, long n) {
    const size_t a = voxel_scatter_det_region_bytes(v->gp), b = voxel_scatter_hybrid_ok(v->gp, n) ? voxel_scatter_hybrid_workspace_bytes(v->gp, n) : 0;
    return a > b ? a : b;
}

static const size_t DET_WS_SLACK = 256;        // alignment slack for an unaligned caller pointer: the region starts at ws_align_ptr(workspace)
size_t evd_voxel_sample_bwd_det_workspace_bytes(const evd_voxel* v, long n) {
    if (!v || n <= 0) return 0;
    return det_region_bytes(v, n) + DET_WS_SLACK;
}

int evd_voxel_sample_bwd_det(const evd_voxel* v, int precision, const float* pts, long n, const float* d_out, int d_stride, int d_col,
                             const evd_voxel_grid_grads* g, float* d_pts, void* workspace, size_t workspace_bytes, void* stream) {
    EVD_REQUIRE(v && pts && d_out && g && n >= 0 && d_stride >= d_col + v->app_dim, "evd_voxel_sample_bwd_det: bad arguments");
    EVD_REQUIRE(precision >= 0 && precision <= EVD_PREC_F16M, "evd_voxel_sample_bwd_det: unknown precision %d", precision);
    EVD_REQUIRE(v->app_act == EVD_ACT_NONE, "evd_voxel_sample_bwd_det: only app_actfn none is built (all shipped configs)");
    if (n == 0) return EVD_OK;
    const size_t need = evd_voxel_sample_bwd_det_workspace_bytes(v, n);
    if (!workspace || workspace_bytes < need) return fail(EVD_E_WORKSPACE, "evd_voxel_sample_bwd_det: workspace %zu < %zu bytes", workspace_bytes, need);
    hipStream_t st = as_stream(stream);
    const bool half = grids_half_for(v, precision);
    const GridGrads gg = grid_grads(g);
    char* region = (char*)ws_align_ptr(workspace);
    int rc = launch_voxel_scatter_det_scale(v->gp, half, pts, n, d_out, d_stride, d_col, gg, region, st);
    if (rc) return rc;
    // the one host read of this entry: the unit is a function of the batch's maximum, and a batch without one takes another path
    unsigned bits = 0;
    EVD_HIP(hipMemcpyAsync(&bits, region, sizeof(bits), hipMemcpyDeviceToHost, st));
    EVD_HIP(hipStreamSynchronize(st));
    float cmax;
    memcpy(&cmax, &bits, sizeof(cmax));
    if (!std::isfinite(cmax))          // a NaN / Inf contribution: no scale exists, the gradients show it as the default path does
        return sample_bwd_ws(v, half, pts, n, d_out, d_stride, d_col, g, d_pts, region, det_region_bytes(v, n), stream);
    return launch_voxel_scatter_det_add(v->gp, half, pts, n, d_out, d_stride, d_col, gg, d_pts, region, evd_scatter_det_unit_exp(cmax, n), st);
}

// the six TV terms of a level: planes at weight 1e-2, lines at 1e-3; g = the gradients they are added to (null: the loss only)
static TvJobs tv_jobs(const evd_voxel* v, const evd_voxel_grid_grads* g) {
    TvJobs jobs;
    jobs.n = 6;
    for (int i = 0; i < 3; ++i) {
        const int C = v->n_comp[i], Wp = v->grid[kMat0[i]], Hp = v->grid[kMat1[i]], Lp = v->grid[kVec[i]];
        jobs.j[i] = TvJob{(const float*)v->plane[i].p, g ? g->plane[i] : nullptr, Hp, Wp, C, 1e-2f, 0, 0};
        jobs.j[3 + i] = TvJob{(const float*)v->line[i].p, g ? g->line[i] : nullptr, Lp, 1, C, 1e-3f, 0, 0};
    }
    return jobs;
}

int evd_voxel_tv_loss_bwd(const evd_voxel* v, const float* d_loss, const evd_voxel_grid_grads* g, void* stream) {
    EVD_REQUIRE(v && g && d_loss, "evd_voxel_tv_loss_bwd: null argument");
    TvJobs jobs = tv_jobs(v, g);
    return launch_tv_bwd_level(jobs, d_loss, as_stream(stream));
}

int evd_voxel_tv_loss(const evd_voxel* v, float* out, void* stream) {
    EVD_REQUIRE(v && out, "evd_voxel_tv_loss: null argument");
    hipStream_t st = as_stream(stream);
    double* acc = (double*)v->tv_acc.p;
    TvShape s;
    TvJobs jobs = tv_jobs(v, nullptr);
    int rc = launch_tv_level(jobs, acc, &s, st);
    if (rc) return rc;
    return launch_tv_finish(acc, s, out, st);
}

}  // extern "C"
