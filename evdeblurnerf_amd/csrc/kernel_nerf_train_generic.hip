// Generic NeRF-mode training (nerf_train_generic.h): the forward kernel that keeps float32 activation rows, and the backward as a chain of
// the per-layer float32 launches of gen_rows.h (dgrad, wgrad + fixed-order reduction, the two encodings).
// reference: the autograd graph of networks/nerf.py:46-72 (mlpforward), :131-162 (eval), networks/embedding.py:88-98.
#include "nerf_train_generic.h"
#include "mlp_device.h"

namespace evd {

// ---------------------------------------------------------------------------------------------------------------------
// Forward: k_nerf_mlp_generic<EVD_PREC_F16X3, W, VKS> (kernel_nerf_mlp.hip) -- the same stream, the same layer<> calls in the same
// order, hence the same raw bit for bit -- with every layer's output written as a float32 row of the store (layer<>'s feat_row).
// A kernel of its own and not a switch in k_nerf_mlp_generic: the inference kernels' code objects stay what they were.
// PDH: where the point encoding's k-steps sit in the skip layer, [h_0 .. h_{PDH-1} | pe | h_PDH .. h_{KS-1}] (nerf_streams.h nerf_layers).  0: the
// generic stream; KS - 2: evd_nerf::stream_pd, the pipelined kernel's order of additions, for the pipelined network's forward with a feature.
template <int W, int VKS, int PDH = 0>
__global__ __launch_bounds__(mlp_threads(EVD_PREC_F16X3), 1) void k_nerf_train_fwd_generic(const MlpParams p) {
    constexpr int PREC = EVD_PREC_F16X3;
    typedef Ops<PREC> O;
    typedef typename O::B B;
    constexpr int NT = mlp_threads(PREC);
    constexpr int T = W / 32, KS = W / 16;
    constexpr int FPC = Stream<PREC>::FPC;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 31, h = lane >> 5;
    const long s = (long)blockIdx.x * (NT / 2) + wave * 32 + n;
    const bool valid = s < p.nsamp;
    const long sc = valid ? s : p.nsamp - 1;
    const long ray = sc / p.S;
    const float* rb = p.ray_batch + ray * p.ncol;
    const float zv = p.z[sc];
    float pts[3], vd[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        pts[c] = __fadd_rn(rb[c], __fmul_rn(rb[3 + c], zv));   // renderer.py:180
        vd[c] = rb[8 + c];
    }
    const GenStore gs(p.nsamp, p.D, W);
    float* const store = reinterpret_cast<float*>(p.act);
    if (valid) {        // the encodings' inputs: lane half 0 the position, half 1 the direction
        const f32x4 v = h ? f32x4{vd[0], vd[1], vd[2], 0.f} : f32x4{pts[0], pts[1], pts[2], 0.f};
        *reinterpret_cast<f32x4*>(store + gs.in() + s * 8 + 4 * h) = v;
    }

    float* bias = stage_bias<PREC>(smem, p.bias, p.nbias, tid);
    B* stash = reinterpret_cast<B*>(smem + MlpLds<PREC>::RING + MlpLds<PREC>::BIAS_FLOATS * 4 + wave * MlpLds<PREC>::STASH_PER_WAVE) + lane;
    B act[KS], nxt[KS];
    {
        B in_pe[PE_KS];
        encode_b_rt<PREC, PE_KS>(pts, h, p.pe_l, in_pe);
#pragma unroll
        for (int j = 0; j < PE_KS; ++j) stash[j * 64] = in_pe[j];
    }
    Stream<PREC> st;
    st.start(p.wstream, smem, p.nchunks, tid);
    float* hrow = valid ? store + gs.h(0) + s * W : nullptr;       // row s of H_0; H_l is nsp * W floats further per layer
    const long hstep = gs.nsp * W;
    {
        B in_pe[PE_KS];
#pragma unroll
        for (int j = 0; j < PE_KS; ++j) in_pe[j] = stash[j * 64];
        layer<PREC, PE_KS, T, true, OUT_B, 0, true>(st, in_pe, nxt, nullptr, bias, lane, hrow, W);
    }
    bias += T * 32;
#pragma unroll
    for (int j = 0; j < KS; ++j) act[j] = nxt[j];

#pragma nounroll
    for (int l = 1; l < p.D; ++l) {
        if (hrow) hrow += hstep;
        if (l - 1 == p.skip) {      // h = cat([input_pts, h]) feeds this layer (nerf.py:137-138)
            B wide[PE_KS + KS];
#pragma unroll
            for (int j = 0; j < PDH; ++j) wide[j] = act[j];
#pragma unroll
            for (int j = 0; j < PE_KS; ++j) wide[PDH + j] = stash[j * 64];
#pragma unroll
            for (int j = PDH; j < KS; ++j) wide[PE_KS + j] = act[j];
            layer<PREC, PE_KS + KS, T, true, OUT_B, 0, true>(st, wide, nxt, nullptr, bias, lane, hrow, W);
        } else {
            layer<PREC, KS, T, true, OUT_B, 0, true>(st, act, nxt, nullptr, bias, lane, hrow, W);
        }
        bias += T * 32;
#pragma unroll
        for (int j = 0; j < KS; ++j) act[j] = nxt[j];
    }

    // heads: alpha_linear (1 tile), feature_linear, views_linears.0 on cat([feature, dirs]), rgb_linear (nerf.py:144-157)
    constexpr int F_ALPHA = KS, F_FEAT = T * KS, F_VIEWS = (T / 2) * (KS + VKS);
    constexpr int OFF_FEAT = F_ALPHA % FPC, OFF_VIEWS = (F_ALPHA + F_FEAT) % FPC, OFF_RGB = (F_ALPHA + F_FEAT + F_VIEWS) % FPC;
    float araw[16], rraw[16];
    layer<PREC, KS, 1, false, OUT_F32, 0, false>(st, act, nullptr, araw, bias, lane, nullptr, W);
    bias += 32;
    layer<PREC, KS, T, false, OUT_B, OFF_FEAT, false>(st, act, nxt, nullptr, bias, lane, valid ? store + gs.f() + s * W : nullptr, W);
    bias += T * 32;
    {
        B vin[KS + VKS];
#pragma unroll
        for (int j = 0; j < KS; ++j) vin[j] = nxt[j];
        {
            B in_dir[VKS];
            encode_b_rt<PREC, VKS>(vd, h, p.pe_lv, in_dir);
#pragma unroll
            for (int j = 0; j < VKS; ++j) vin[KS + j] = in_dir[j];
        }
        layer<PREC, KS + VKS, T / 2, true, OUT_B, OFF_VIEWS, false>(st, vin, act, nullptr, bias, lane, valid ? store + gs.hv() + s * (W / 2) : nullptr, W);
        bias += (T / 2) * 32;
    }
    {
        B hin[KS / 2];
#pragma unroll
        for (int j = 0; j < KS / 2; ++j) hin[j] = act[j];
        layer<PREC, KS / 2, 1, false, OUT_F32, OFF_RGB, true>(st, hin, nullptr, rraw, bias, lane, nullptr, W);
    }
    if (h == 0 && valid) {
        const f32x4 o = {rraw[0], rraw[1], rraw[2], araw[0]};   // cat([rgb, alpha]) nerf.py:157
        *reinterpret_cast<f32x4*>(p.raw + s * 4) = o;
    }
}

template <int W, int VKS, int PDH = 0>
static int launch_fwd(const MlpParams& p, hipStream_t st) {
    constexpr int PREC = EVD_PREC_F16X3, NT = mlp_threads(PREC);
    const long blocks = cdiv(p.nsamp, NT / 2);
    const size_t lds = MlpLds<PREC>::TOTAL;
    EVD_SET_MAX_LDS((&k_nerf_train_fwd_generic<W, VKS, PDH>), lds);
    if (p.nbias > MlpLds<PREC>::BIAS_FLOATS) return fail(EVD_E_INVALID, "evd_nerf_mlp_train: %d bias floats exceed the LDS bias block", p.nbias);
    hipLaunchKernelGGL((k_nerf_train_fwd_generic<W, VKS, PDH>), dim3((unsigned)blocks), dim3(NT), lds, st, p);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int launch_nerf_train_fwd_generic(int W, const MlpParams& p, hipStream_t st, int pdh) {
    const bool widev = pe_ksteps(p.pe_lv) > 2;
    if (pdh) {          // the pipelined network's stream_pd: one shape
        if (W == 256 && !widev && pdh == 14) return launch_fwd<256, 2, 14>(p, st);      // (10, 4): two direction k-steps
        return fail(EVD_E_INVALID, "evd_nerf_mlp_train_feature: no training kernel for the skip layer order %d at width %d", pdh, W);
    }
    if (W == 64) return widev ? launch_fwd<64, 4>(p, st) : launch_fwd<64, 2>(p, st);
    if (W == 128) return widev ? launch_fwd<128, 4>(p, st) : launch_fwd<128, 2>(p, st);
    if (W == 256) return widev ? launch_fwd<256, 4>(p, st) : launch_fwd<256, 2>(p, st);
    return fail(EVD_E_INVALID, "evd_nerf_mlp_train: no generic training kernel for width %d (built: 64, 128, 256)", W);
}

// ---------------------------------------------------------------------------------------------------------------------
// Backward: the per-layer launches of gen_rows.h, and the one step that is this network's own.
// d pre-activation of views_linears.0 from d rgb (rgb_linear has three rows: no matrix core needed).  thread = 4 columns of one sample.
__global__ __launch_bounds__(256) void k_gen_rgb_dgrad(const float* __restrict__ d_raw, const float* __restrict__ rgb_w, const float* __restrict__ hv,
                                                       long nsamp, int H, float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int per = H / 4;
    const long s = i / per;
    if (s >= nsamp) return;
    const int k = (int)(i % per) * 4;
    const f32x4 g = *reinterpret_cast<const f32x4*>(d_raw + s * 4);
    const f32x4 m = *reinterpret_cast<const f32x4*>(hv + s * H + k);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float x = g[0] * rgb_w[k + e] + g[1] * rgb_w[H + k + e] + g[2] * rgb_w[2 * H + k + e];
        o[e] = m[e] > 0.f ? x : 0.f;
    }
    *reinterpret_cast<f32x4*>(out + s * H + k) = o;
}

int run_nerf_backward_generic(const GenBwdPlan& b, hipStream_t st) {
    const evd_nerf* net = b.net;
    const int D = net->D, W = net->W, H = W / 2, L = net->multires, Lv = net->multires_views;
    const int IC = 3 * (1 + 2 * L), ICV = 3 * (1 + 2 * Lv);
    const long n = b.nsamp;
    if (!net->params_f32.p) return fail(EVD_E_INVALID, "evd_nerf_mlp_backward: the handle holds no float32 parameters for the generic training path");
    const GenStore gs(n, D, W);
    float* S = b.store;
    const float* P = (const float*)net->params_f32.p;
    auto par = [&](int i) { return P + net->param_off[i]; };
    const float *views_w = par(2 * D), *feature_w = par(2 * D + 2), *alpha_w = par(2 * D + 4), *rgb_w = par(2 * D + 6);
    float *ep = S + gs.enc(0), *ed = S + gs.enc(1), *dep = S + gs.enc(2), *ded = S + gs.enc(3);
    float *g0 = S + gs.g(0), *g1 = S + gs.g(1);
    auto hrow = [&](int l) { return (const float*)(S + gs.h(l)); };
    const float *frow = S + gs.f(), *hv = S + gs.hv();

    if (int rc = launch_gen_encode(S + gs.in(), n, L, Lv, ep, ed, st)) return rc;
    GenChain c{n, b.partial, b.accumulate, st, "evd_nerf_mlp_backward"};

    // rgb_linear on hv (nerf.py:155-156)
    c.wgrad(b.d_raw, 4, 3, hv, H, H, b.grads.rgb_w, H, 0, b.grads.rgb_b);
    hipLaunchKernelGGL(k_gen_rgb_dgrad, dim3((unsigned)cdiv(n * (H / 4), 256)), dim3(256), 0, st, b.d_raw, rgb_w, hv, n, H, g0);
    EVD_LAUNCH_CHECK();
    // views_linears.0 on cat([feature, PE(dirs)]) (nerf.py:151-154); g0 = d its pre-activation [n, H]
    c.wgrad(g0, H, H, frow, W, W, b.grads.views_w, W + ICV, 0, b.grads.views_b);
    c.wgrad(g0, H, H, ed, GEN_ENC, ICV, b.grads.views_w, W + ICV, W, nullptr);
    const bool fg1 = b.d_feature && b.feature_kind == 1, fg2 = b.d_feature && b.feature_kind == 2;
    auto rows_in = [&](const float* mask, float* out) { return launch_gen_rows_in(b.d_feature, b.ldf, mask, n, W, out, st); };
    if (fg1)
        if (int rc = rows_in(nullptr, g1)) return rc;
    c.dgrad(H, g0, H, views_w, W + ICV, 0, W, g1, W, nullptr, 0, nullptr, nullptr, fg1 ? 1 : 0);          // g1 = d feature
    if (b.d_dirs) c.dgrad(H, g0, H, views_w, W + ICV, W, ICV, ded, GEN_ENC, nullptr, 0, nullptr, nullptr, 0);
    // feature_linear and alpha_linear on h_{D-1} (nerf.py:144-150)
    c.wgrad(g1, W, W, hrow(D - 1), W, W, b.grads.feature_w, W, 0, b.grads.feature_b);
    c.wgrad(b.d_raw + 3, 4, 1, hrow(D - 1), W, W, b.grads.alpha_w, W, 0, b.grads.alpha_b);
    if (fg2)
        if (int rc = rows_in(hrow(D - 1), g0)) return rc;
    c.dgrad(W, g1, W, feature_w, W, 0, W, g0, W, hrow(D - 1), W, b.d_raw + 3, alpha_w, fg2 ? 1 : 0);      // g0 = d pre-activation of pts_linears[D-1]
    // the trunk, last layer first; cur = d pre-activation of layer l
    float *cur = g0, *oth = g1;
    int pe_written = 0;
    for (int l = D - 1; l >= 0; --l) {
        const float* wl = par(2 * l);
        if (l == 0) {
            c.wgrad(cur, W, W, ep, GEN_ENC, IC, b.grads.pts_w[0], IC, 0, b.grads.pts_b[0]);
            if (b.d_pts) c.dgrad(W, cur, W, wl, IC, 0, IC, dep, GEN_ENC, nullptr, 0, nullptr, nullptr, pe_written);
            break;
        }
        const bool wide = l - 1 == net->skip;       // the layer reads cat([PE(pts), h_{l-1}]) (nerf.py:137-138)
        const int in = wide ? IC + W : W, hc0 = wide ? IC : 0;
        c.wgrad(cur, W, W, hrow(l - 1), W, W, b.grads.pts_w[l], in, hc0, b.grads.pts_b[l]);
        if (wide) {
            c.wgrad(cur, W, W, ep, GEN_ENC, IC, b.grads.pts_w[l], in, 0, nullptr);
            if (b.d_pts) { c.dgrad(W, cur, W, wl, in, 0, IC, dep, GEN_ENC, nullptr, 0, nullptr, nullptr, 0); pe_written = 1; }
        }
        c.dgrad(W, cur, W, wl, in, hc0, W, oth, W, hrow(l - 1), W, nullptr, nullptr, 0);
        float* t = cur; cur = oth; oth = t;
    }
    if (c.rc) return c.rc;
    if (b.d_pts)
        if (int rc = launch_gen_encode_bwd(ep, dep, n, L, b.d_pts, st)) return rc;
    if (b.d_dirs)
        if (int rc = launch_gen_encode_bwd(ed, ded, n, Lv, b.d_dirs, st)) return rc;
    return EVD_OK;
}

}  // namespace evd
