// The weight streams of an evd_nerf handle (nerf_net.h), built by evd_nerf_create: the layer tables of the generic, the pipelined and the
// compensated kernels, the W^T streams of the training backward, the wgrad index maps and the bias image.  Every function reads the
// network's shape and parameter offsets from the handle and the weights from the host arena A; the arrangements are frag_layout.h's.
#pragma once

#include "frag_layout.h"
#include "nerf_net.h"
#include "nerf_train.h"

namespace evd {

// the head's parameter blocks behind the 2 D blocks of pts_linears ({weight, bias} each; a use_viewdirs=False network: output_linear at 0)
enum { NB_VIEWS = 0, NB_FEATURE = 2, NB_ALPHA = 4, NB_RGB = 6, NB_OUTPUT = 0 };

struct NerfDims {
    const int D, W, T = W / 32, KS = W / 16, L, Lv, IC = 3 * (1 + 2 * L), ICV = 3 * (1 + 2 * Lv), head = 2 * D;
    explicit NerfDims(const evd_nerf& n) : D(n.D), W(n.W), L(n.multires), Lv(n.multires_views) {}
};

// The layer table of k_nerf_mlp (pdh = 0) and of the pipelined kernel (nerf_mlp_kernel.h): the skip layer's k-steps are
// [h_0..h_{pdh-1} | pe_0..3 | h_pdh..h_{KS-1}].  out_rows: the rows of output_linear that raw2outputs reads
inline void nerf_layers(StreamBuilder& sb, const evd_nerf& n, const float* A, int out_rows, int pdh) {
    const NerfDims s(n);
    const int D = s.D, W = s.W, T = s.T, KS = s.KS, VKS = pe_ksteps(s.Lv) <= 2 ? 2 : 4;
    auto P = [&](int i) { return A + n.param_off[i]; };
    sb.layer(P(0), W, s.IC, T, PE_KS, true, pe_at(s.L, 0));
    for (int l = 1; l < D; ++l) {
        if (l - 1 == n.skip) sb.layer(P(2 * l), W, W + s.IC, T, PE_KS + KS, true, wide_col(pdh, s.L, s.IC, hid_col));
        else sb.layer(P(2 * l), W, W, T, KS, true, hid_col);
    }
    if (n.no_views) {
        sb.layer(P(s.head + NB_OUTPUT), out_rows, W, 1, KS, true, hid_col);
        return;
    }
    sb.layer(P(s.head + NB_ALPHA), 1, W, 1, KS, false, hid_col);
    sb.layer(P(s.head + NB_FEATURE), W, W, T, KS, false, hid_col);
    sb.layer(P(s.head + NB_VIEWS), W / 2, W + s.ICV, T / 2, KS + VKS, false, lead_then_pe(KS, hid_col, s.Lv, W));
    sb.layer(P(s.head + NB_RGB), 3, W / 2, 1, KS / 2, true, hid_col);
}

// The compensated mode's table (nerf_mlp_c_kernel.h): groups of two tiles, 64-input blocks, the skip layer's blocks
// [h_0 .. h_{KB-2} | pe | h_{KB-1}].  fold: the inference stream -- no feature layer, views_linears.0 replaced by the folded layer, whose
// elements live behind the parameters in the extended arena (evd_api.hip k_fold_feature); base: the arena the source maps index
inline void nerf_layers_c(StreamBuilderC& sc, const evd_nerf& n, const float* base, bool fold) {
    const NerfDims s(n);
    const int D = s.D, W = s.W, T = s.T, KS = s.KS, KB = KS / 4;
    auto P = [&](int i) { return base + n.param_off[i]; };
    sc.arena = base;
    sc.layer(P(0), W, s.IC, T, PE_KS, 2, pe_at(s.L, 0));
    for (int l = 1; l < D; ++l) {
        if (l - 1 == n.skip) sc.layer(P(2 * l), W, W + s.IC, T, PE_KS + KS, 2, wide_col(4 * (KB - 1), s.L, s.IC, c_hid_col));
        else sc.layer(P(2 * l), W, W, T, KS, 2, c_hid_col);
    }
    sc.layer(P(s.head + NB_ALPHA), 1, W, 1, KS, 1, c_hid_col);
    if (!fold) sc.layer(P(s.head + NB_FEATURE), W, W, T, KS, 2, c_hid_col);
    sc.layer(fold ? base + n.param_off[n.nparam_blocks] : P(s.head + NB_VIEWS), W / 2, W + s.ICV, T / 2, KS + PEV_KS, 2,
             lead_then_pe(KS, c_hid_col, s.Lv, W));
    sc.layer(P(s.head + NB_RGB), 3, W / 2, 1, KS / 2, 1, c_hid_col);
}

// The W^T streams of the dgrad chain in mode prec, one per layer (nerf_train_kernel.h), and the encoding rows for the gradient w.r.t.
// the rays
inline int nerf_wt_streams(evd_nerf& n, int prec, const float* A) {
    const NerfDims s(n);
    const int D = s.D, W = s.W, T = s.T, KS = s.KS, IC = s.IC, ICV = s.ICV;
    auto P = [&](int i) { return A + n.param_off[i]; };
    auto put = [&](int which, auto fill) { return put_wt(n.bwd[prec][which], prec, A, fill); };
    int rc = put(EVD_BWD_RGB, [&](StreamBuilder& b) { b.layer_transposed(P(s.head + NB_RGB), 3, W / 2, 0, W / 2, nullptr, 0, T / 2, 1, true, nat_col(3)); });
    if (!rc) rc = put(EVD_BWD_VIEWS, [&](StreamBuilder& b) { b.layer_transposed(P(s.head + NB_VIEWS), W / 2, W + ICV, 0, W, nullptr, 0, T, KS / 2, true, hid_col); });
    if (!rc) rc = put(EVD_BWD_HEAD, [&](StreamBuilder& b) {        // [feature_linear | alpha_linear]^T
        b.layer_transposed(P(s.head + NB_FEATURE), W, W, 0, W, P(s.head + NB_ALPHA), 1, T, KS + 1, true, lead_then_one(KS, hid_col, W));
    });
    if (!rc) rc = put(EVD_BWD_PE0, [&](StreamBuilder& b) { enc_layer_wt(b, P(0), IC, 0, 0, PE_L, 2, KS); });
    if (!rc && n.skip >= 0 && n.skip + 1 < D) rc = put(EVD_BWD_PESKIP, [&](StreamBuilder& b) { enc_layer_wt(b, P(2 * (n.skip + 1)), W + IC, 0, 0, PE_L, 2, KS); });
    if (!rc) rc = put(EVD_BWD_DIR, [&](StreamBuilder& b) { enc_layer_wt(b, P(s.head + NB_VIEWS), W + ICV, 0, W, PE_LV, 1, KS / 2); });
    for (int l = 1; l < D && !rc; ++l) {
        const bool wide = l - 1 == n.skip;
        rc = put(EVD_BWD_HIDDEN1 + l - 1, [&](StreamBuilder& b) { b.layer_transposed(P(2 * l), W, wide ? W + IC : W, wide ? IC : 0, W, nullptr, 0, T, KS, true, hid_col); });
    }
    return rc;
}

// wgrad index maps (nerf_train.h): fragment column -> parameter row / column
inline std::vector<int> nerf_wgrad_maps(const evd_nerf& n) {
    const NerfDims s(n);
    std::vector<int> m(MAP_TOTAL, -1);
    fill_map(m, MAP_HID, 256, hid_col);
    fill_map(m, MAP_HID_SKIP, 256, offset(s.IC, hid_col));
    fill_map(m, MAP_PE, 64, pe_at(s.L, 0));
    fill_map(m, MAP_DIR, 32, pe_at(s.Lv, s.W));
    fill_map(m, MAP_RGB, 3, nat_col(3));
    m[MAP_ALPHA] = 0;
    return m;
}

// biases, one 32-float row block per output tile, in stream order
inline BiasImage nerf_bias_image(const evd_nerf& n, const float* A, int out_rows) {
    const NerfDims s(n);
    BiasImage b(A, n.param_off);
    for (int l = 0; l < s.D; ++l) b.push(2 * l + 1, s.W, s.T);
    if (n.no_views) {
        b.push(s.head + NB_OUTPUT + 1, out_rows, 1);
    } else {
        b.push(s.head + NB_ALPHA + 1, 1, 1);
        b.push(s.head + NB_FEATURE + 1, s.W, s.T);
        b.push(s.head + NB_VIEWS + 1, s.W / 2, s.T / 2);
        b.push(s.head + NB_RGB + 1, 3, 1);
    }
    return b;
}

}  // namespace evd
