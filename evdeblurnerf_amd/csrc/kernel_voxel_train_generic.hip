// Backward of a generic PDRF level (voxel_generic.h), EVD_PREC_F16X3: per layer one wgrad and one dgrad launch of the float32-row kernels
// (gen_rows.h GenChain: exact float32 on the matrix cores, per-wavefront partials folded in a fixed order, the parameters read
// in place from the handle's float32 copy; no floating-point atomics, no host synchronisation).
// reference: the autograd graph of networks/pdrf/voxnerf.py:210-221 (sigma net), :240-254 (colour net), networks/embedding.py:88-98.
#include "voxel_generic.h"
#include "gen_rows.h"
#include "mlp_device.h"

namespace evd {

// The heads' gradient rows.  dcol[s, k] = d raw[s, 1 + k] y (1 - y), y = raw[s, 1 + k] = sigmoid(colour pre-activation) (voxnerf.py:252),
// zero from column 3 on; dgeo[s, c] = d_feature[s, c] (or zero), zero from column G on.  thread = 4 columns of one sample, 160 columns.
__global__ __launch_bounds__(256) void k_voxgen_heads(const float* __restrict__ d_raw, const float* __restrict__ raw, const float* __restrict__ d_feature, int G,
                                                      long nsamp, float* __restrict__ dgeo, float* __restrict__ dcol) {
    constexpr int PER = (VG_GEO_LD + VG_COL_LD) / 4;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long s = i / PER;
    if (s >= nsamp) return;
    const int k = (int)(i % PER) * 4;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (k < VG_GEO_LD) {
        if (d_feature) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (k + e < G) o[e] = d_feature[s * G + k + e];
        }
        *reinterpret_cast<f32x4*>(dgeo + s * VG_GEO_LD + k) = o;
    } else {
        if (k == VG_GEO_LD) {
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const float y = raw[s * 4 + 1 + e];
                o[e] = d_raw[s * 4 + 1 + e] * (y * (1.f - y));
            }
        }
        *reinterpret_cast<f32x4*>(dcol + s * VG_COL_LD + (k - VG_GEO_LD)) = o;
    }
}

// rows of a staging plane to the caller's d_fts rows.  thread = 4 columns of one sample (FT is a multiple of 16).
__global__ __launch_bounds__(256) void k_voxgen_rows_out(const float* __restrict__ src, int lds, int FT, long nsamp, float* __restrict__ dst, int ldd) {
    const int per = FT / 4;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long s = i / per;
    if (s >= nsamp) return;
    const int k = (int)(i % per) * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) dst[s * ldd + k + e] = src[s * lds + k + e];
}

int run_voxel_backward_generic(const VoxGenBwdPlan& b, hipStream_t st) {
    const int HD = b.HD, G = b.G, FT = b.FT, NS = b.NS, NC = b.NC;
    const int IC = 3 * (1 + 2 * b.L), ICV = 3 * (1 + 2 * b.Lv), IN0 = FT + IC, CIN = G + ICV;
    const long n = b.nsamp;
    const VoxGenStore gs(n, HD, NS, NC);
    float* S = b.store;
    auto sig_w = [&](int l) { return b.params + b.off[l]; };
    auto col_w = [&](int l) { return b.params + b.off[NS + 2 * l]; };
    const float *fts = S + gs.fts(), *geo = S + gs.geo();
    float *ep = S + gs.enc(0), *ed = S + gs.enc(1), *dep = S + gs.enc(2), *ded = S + gs.enc(3);
    float *dgeo = S + gs.dgeo(), *dcol = S + gs.dcol();
    float *cur = S + gs.g(0), *oth = S + gs.g(1);
    auto swap = [&]() { float* t = cur; cur = oth; oth = t; };
    const int MG = G <= 32 ? 32 : G <= 64 ? 64 : 128;       // the dgrad kernel's gradient columns for the geo rows

    hipLaunchKernelGGL(k_voxgen_heads, dim3((unsigned)cdiv(n * ((VG_GEO_LD + VG_COL_LD) / 4), 256)), dim3(256), 0, st, b.d_raw, b.raw, b.d_feature, G, n, dgeo, dcol);
    EVD_LAUNCH_CHECK();
    if (int rc = launch_gen_encode(S + gs.in(), n, b.L, b.Lv, ep, ed, st)) return rc;
    GenChain c{n, b.partial, b.accumulate, st, "evd_voxel_mlp_backward"};

    // ---- colour net, last layer first (voxnerf.py:248-252); G_ = d pre-activation of layer l: [n, M] rows of ldg floats
    {
        const float* G_ = dcol;
        int ldg = VG_COL_LD, M = 3, MT = 32;
        for (int l = NC - 1; l >= 0; --l) {
            if (l == 0) {       // reads cat([geo, PE(dirs)])
                c.wgrad(G_, ldg, M, geo, VG_GEO_LD, G, b.color_w[0], CIN, 0, b.color_b[0]);
                c.wgrad(G_, ldg, M, ed, GEN_ENC, ICV, b.color_w[0], CIN, G, nullptr);
                c.dgrad(MT, G_, ldg, col_w(0), CIN, 0, G, dgeo, VG_GEO_LD, nullptr, 0, nullptr, nullptr, 1, M);
                if (b.d_dirs) c.dgrad(MT, G_, ldg, col_w(0), CIN, G, ICV, ded, GEN_ENC, nullptr, 0, nullptr, nullptr, 0, M);
                break;
            }
            const float* x = S + gs.hc(l - 1);
            c.wgrad(G_, ldg, M, x, HD, HD, b.color_w[l], HD, 0, b.color_b[l]);
            c.dgrad(MT, G_, ldg, col_w(l), HD, 0, HD, oth, HD, x, HD, nullptr, nullptr, 0, M);
            swap();
            G_ = cur; ldg = HD; M = HD; MT = HD;
        }
    }
    // ---- sigma net (voxnerf.py:214-218): the last layer's gradient rows are [d sigma = d raw[:, 0] | dgeo]
    {
        const float* wl = sig_w(NS - 1);
        const int in = NS == 1 ? IN0 : HD;
        float* dw = b.sigma_w[NS - 1];
        // the input planes of a layer that reads cat([fts, PE(pts)]) (layer 0), as column pieces (plane, row stride, columns, first column)
        auto wgrad_in0 = [&](const float* G_, int ldg, int M, float* dwp) {
            c.wgrad(G_, ldg, M, fts, VG_FT_LD, FT, dwp, IN0, 0, nullptr);
            c.wgrad(G_, ldg, M, ep, GEN_ENC, IC, dwp, IN0, FT, nullptr);
        };
        if (NS == 1) {
            wgrad_in0(b.d_raw, 4, 1, dw);
            wgrad_in0(dgeo, VG_GEO_LD, G, dw ? dw + in : nullptr);
            if (b.d_fts) c.dgrad(MG, dgeo, VG_GEO_LD, wl + in, in, 0, FT, cur, HD, nullptr, 0, b.d_raw, wl, 0, G);
            if (b.d_pts) c.dgrad(MG, dgeo, VG_GEO_LD, wl + in, in, FT, IC, dep, GEN_ENC, nullptr, 0, b.d_raw, wl + FT, 0, G);
        } else {
            const float* x = S + gs.hs(NS - 2);
            c.wgrad(b.d_raw, 4, 1, x, HD, HD, dw, HD, 0, nullptr);
            c.wgrad(dgeo, VG_GEO_LD, G, x, HD, HD, dw ? dw + in : nullptr, HD, 0, nullptr);
            c.dgrad(MG, dgeo, VG_GEO_LD, wl + in, in, 0, HD, cur, HD, x, HD, b.d_raw, wl, 0, G);
            for (int l = NS - 2; l >= 0; --l) {     // cur = d pre-activation of sigma_net.l
                if (l == 0) {
                    wgrad_in0(cur, HD, HD, b.sigma_w[0]);
                    if (b.d_pts) c.dgrad(HD, cur, HD, sig_w(0), IN0, FT, IC, dep, GEN_ENC, nullptr, 0, nullptr, nullptr, 0);
                    if (b.d_fts) { c.dgrad(HD, cur, HD, sig_w(0), IN0, 0, FT, oth, HD, nullptr, 0, nullptr, nullptr, 0); swap(); }
                    break;
                }
                const float* xl = S + gs.hs(l - 1);
                c.wgrad(cur, HD, HD, xl, HD, HD, b.sigma_w[l], HD, 0, nullptr);
                c.dgrad(HD, cur, HD, sig_w(l), HD, 0, HD, oth, HD, xl, HD, nullptr, nullptr, 0);
                swap();
            }
        }
    }
    if (c.rc) return c.rc;
    if (b.d_fts) {      // cur holds d fts in rows of HD floats (the dgrad writes whole 32-column blocks: staged, then cut to the caller's rows)
        hipLaunchKernelGGL(k_voxgen_rows_out, dim3((unsigned)cdiv(n * (FT / 4), 256)), dim3(256), 0, st, (const float*)cur, HD, FT, n, b.d_fts, b.d_fts_stride);
        EVD_LAUNCH_CHECK();
    }
    if (b.d_pts)
        if (int rc = launch_gen_encode_bwd(ep, dep, n, b.L, b.d_pts, st)) return rc;
    if (b.d_dirs)
        if (int rc = launch_gen_encode_bwd(ed, ded, n, b.Lv, b.d_dirs, st)) return rc;
    return EVD_OK;
}

}  // namespace evd
