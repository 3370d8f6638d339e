// Backward of the fused NeRF MLP (bf16 / f16 modes, netdepth 8, netwidth 256, skips [4]).
// reference: the autograd graph of NeRF.mlpforward, networks/nerf.py:46-72, differentiated by run_nerf.py:593-601.
//
// Everything works on the activation store the training forward filled (nerf_mlp.h, namespace astore): one 1 KiB MFMA
// B fragment per (32-sample tile, 16 channels), lane-linear, so every access below is a coalesced 16-byte load/store
// per lane and no kernel ever re-arranges data through LDS.
//
//   nerf_bwd_frags.h   k_grad_frags: d raw [n,4] (float32) x 2^s -> the two gradient fragments G_RGB, G_ALPHA (s: power-of-two loss scale
//                      that puts max |d raw| in [512, 1024), so float16 gradients neither overflow nor flush); k_pe_bwd
//   nerf_bwd_dgrad.h   k_dgrad_layer: d x = (W^T d y) . [x > 0] for ONE layer, on the software pipeline of the forward kernel
//   nerf_bwd_wgrad.h   k_wgrad / k_wgrad_split: dW = d y . x^T over all samples, blocks transposed on the matrix core (bwd_tile.h)
//   nerf_bwd_fused.h   k_wgrad_dgrad / k_wgrad_dgrad_p: wgrad and dgrad of a 256-wide layer in one launch
//   nerf_bwd_reduce.h  k_wgrad_reduce: sums the partials, undoes the fragment permutations through two index maps, removes the loss scale
// This file: run_nerf_backward, the whole backward of one network.
#pragma once

#include "nerf_bwd_dgrad.h"
#include "nerf_bwd_frags.h"
#include "nerf_bwd_fused.h"
#include "nerf_bwd_reduce.h"
#include "nerf_bwd_wgrad.h"
#include "bwd_launch.h"

namespace evd {

// The whole backward of one network, in the order the gradients become available.
template <int PREC> static int run_nerf_backward(const BwdPlan& b, hipStream_t st) {
    using namespace astore;
    constexpr int D = 8;
    int rc;
    EVD_HIP(hipMemsetAsync(b.maxbits, 0, sizeof(unsigned), st));
    hipLaunchKernelGGL(k_absmax, dim3(512), dim3(256), 0, st, b.d_raw, b.nsamp * 4, b.maxbits);
    EVD_LAUNCH_CHECK();
    hipLaunchKernelGGL((k_grad_frags<PREC>), dim3((unsigned)cdiv(b.tiles * 64, 256L)), dim3(256), 0, st, b.d_raw, b.nsamp, b.maxbits, b.store, b.tiles);
    EVD_LAUNCH_CHECK();

    const BwdChain c(b, astore::tile_bytes(PREC), st);
    const int wb = c.tile_grid();
    auto dgrad = [&](int stream, int in_slot, int extra_slot, int mask_slot, int out_slot) { return c.dgrad_params(b.wt[stream], in_slot, extra_slot, mask_slot, out_slot); };
    const BwdGrads& g = b.grads;
    // Every wgrad is issued BEFORE the dgrad layer that reads the same two arrays (BwdChain::wgrad; the side stream is b.side: developer
    // switch EVD_BWD_OVERLAP).
    // rgb_linear: d hv = Wr^T d rgb;  dWr = d rgb . hv^T
    if ((rc = c.wgrad(launch_wgrad<PREC, 1, 4, true>, wb, 1, 4, true, G_RGB, HV, MAP_RGB, MAP_HID, g.rgb_w, 128, g.rgb_b))) return rc;
    if ((rc = launch_dgrad<PREC, 1, 4, 1, false, 2>(dgrad(EVD_BWD_RGB, G_RGB, -1, M_HV, D_HV), b.tiles, st))) return rc;
    // views_linears.0 on cat([feature, PE(dir)])
    if ((rc = c.wgrad(launch_wgrad<PREC, 4, 8, false>, wb, 4, 8, true, D_HV, F, MAP_HID, MAP_HID, g.views_w, 256 + 27, g.views_b))) return rc;
    if ((rc = c.wgrad(launch_wgrad<PREC, 4, 1, false>, wb, 4, 1, false, D_HV, DIR, MAP_HID, MAP_DIR, g.views_w, 256 + 27, nullptr))) return rc;
    if ((rc = launch_dgrad<PREC, 8, 8, 8, false, 0>(dgrad(EVD_BWD_VIEWS, D_HV, -1, -1, D_F), b.tiles, st))) return rc;
    // feature_linear and alpha_linear both read h_7
    if ((rc = c.wgrad(launch_wgrad<PREC, 8, 8, false>, wb, 8, 8, true, D_F, H0 + 16 * (D - 1), MAP_HID, MAP_HID, g.feature_w, 256, g.feature_b))) return rc;
    if ((rc = c.wgrad(launch_wgrad<PREC, 1, 8, true>, wb, 1, 8, true, G_ALPHA, H0 + 16 * (D - 1), MAP_ALPHA, MAP_HID, g.alpha_w, 256, g.alpha_b))) return rc;
    if ((rc = launch_dgrad<PREC, 17, 8, 16, true, 2>(dgrad(EVD_BWD_HEAD, D_F, G_ALPHA, M_H0 + D - 1, D_H0 + 16 * (D - 1)), b.tiles, st))) return rc;
    // pts_linears[l], l = 7 .. 1
    for (int l = D - 1; l >= 1; --l) {
        const bool wide = l - 1 == b.skip;
        if constexpr (is_half_prec(PREC)) {
            if (g.pts_w[l]) {           // wgrad(l) with dgrad(l) in one launch (k_wgrad_dgrad above): the seven 256 x 256 trunk layers in the half-precision modes
                if (wide && (rc = c.wgrad(launch_wgrad<PREC, 8, 2, false>, wb, 8, 2, false, D_H0 + 16 * l, PE, MAP_HID, MAP_PE, g.pts_w[l], 256 + 63, nullptr))) return rc;
                if ((rc = c.fused(launch_wgrad_dgrad<PREC, 8, 8, 1>, 8, true, D_H0 + 16 * l, H0 + 16 * (l - 1), MAP_HID, wide ? MAP_HID_SKIP : MAP_HID, g.pts_w[l],
                                  wide ? 256 + 63 : 256, g.pts_b[l], b.wt[EVD_BWD_HIDDEN1 + l - 1], D_H0 + 16 * (l - 1)))) return rc;
                continue;
            }
        }
        if ((rc = c.wgrad(launch_wgrad<PREC, 8, 8, false>, wb, 8, 8, true, D_H0 + 16 * l, H0 + 16 * (l - 1), MAP_HID, wide ? MAP_HID_SKIP : MAP_HID,
                          g.pts_w[l], wide ? 256 + 63 : 256, g.pts_b[l]))) return rc;
        if (wide && (rc = c.wgrad(launch_wgrad<PREC, 8, 2, false>, wb, 8, 2, false, D_H0 + 16 * l, PE, MAP_HID, MAP_PE, g.pts_w[l], 256 + 63, nullptr))) return rc;
        if ((rc = launch_dgrad<PREC, 16, 8, 16, false, 2>(dgrad(EVD_BWD_HIDDEN1 + l - 1, D_H0 + 16 * l, -1, M_H0 + l - 1, D_H0 + 16 * (l - 1)), b.tiles, st))) return rc;
    }
    // gradient w.r.t. the rays: the encoding rows of pts_linears[0], of the skip layer and of views_linears.0, then through sin / cos
    if (b.d_pts) {
        if ((rc = launch_dgrad<PREC, 16, 2, 16, false, 0>(dgrad(EVD_BWD_PE0, D_H0, -1, -1, D_PE0), b.tiles, st))) return rc;
        if ((rc = c.template pe_bwd<PREC, PE_L, PE_KS>(D_PE0, b.pts, 3, 1, b.d_pts, 0))) return rc;
        if (b.skip >= 0 && b.skip + 1 < D) {
            if ((rc = launch_dgrad<PREC, 16, 2, 16, false, 0>(dgrad(EVD_BWD_PESKIP, D_H0 + 16 * (b.skip + 1), -1, -1, D_PE5), b.tiles, st))) return rc;
            if ((rc = c.template pe_bwd<PREC, PE_L, PE_KS>(D_PE5, b.pts, 3, 1, b.d_pts, 1))) return rc;
        }
    }
    if (b.d_dirs) {
        if ((rc = launch_dgrad<PREC, 8, 1, 8, false, 0>(dgrad(EVD_BWD_DIR, D_HV, -1, -1, D_DIRG), b.tiles, st))) return rc;
        if ((rc = c.template pe_bwd<PREC, PE_LV, PEV_KS>(D_DIRG, b.viewdirs, b.vd_stride, b.S, b.d_dirs, 0))) return rc;
    }
    // pts_linears[0] on PE(pts) (no dgrad beyond the inputs)
    if ((rc = c.wgrad(launch_wgrad<PREC, 8, 2, false>, wb, 8, 2, true, D_H0, PE, MAP_HID, MAP_PE, g.pts_w[0], 63, g.pts_b[0]))) return rc;
    return c.join();
}

}  // namespace evd
