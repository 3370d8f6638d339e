// The weight streams of an evd_voxel handle (voxel_net.h), built by evd_voxel_create: the layer tables of k_voxel_mlp, of the pipelined /
// resident kernels (VoxNet), of the generic level's kernel and of the compensated kernel (VoxNetC), the W^T streams of the training
// backward and the wgrad index maps.  Every function reads the level's shape and parameter offsets from the handle and the weights from the
// host arena A; the arrangements are frag_layout.h's.  Layer shapes: voxnerf.py:48-82 (the colour network's hidden width is hidden_dim,
// :73,78); color_net.0 reads cat([h[..., 1:], PE(dirs)]) (:248), sigma_net.0 cat([fts, PE(pts)]).
#pragma once

#include "frag_layout.h"
#include "voxel_net.h"

namespace evd {

struct VoxDims {
    const int NS, NC, HD, G, FT, L, Lv, T = HD / 32, KS = HD / 16, KF = FT / 16, GT = (G + 31) / 32, GK = 2 * GT, ICV = 3 * (1 + 2 * Lv);
    explicit VoxDims(const evd_voxel& v) : NS(v.num_layers), NC(v.num_layers_color), HD(v.hidden_dim), G(v.geo), FT(v.ft_dim), L(v.multires), Lv(v.multires_views) {}
};

// sigma_net (its last layer as the density tile, then the geo rows in GT zero-padded one-tile layers) and color_net, stated once for
//   the VoxNet table of a standard level (voxel_mlp_kernel.h):  kf = KF feature and gk = GK geo k-steps, padded at the end only, a builder of
//                                                               single-tile groups (the geo tiles are then ONE layer of that table);
//   the generic level's table (kernel_voxel_generic.hip):       kf = VG_KF, gk = VG_GK (absent channels: zero), every layer padded.
inline void voxel_layers(StreamBuilder& sb, const evd_voxel& v, const float* A, int kf, int gk, bool pad_each) {
    const VoxDims s(v);
    auto in0 = lead_then_pe(kf, nat_col(s.FT), s.L, s.FT);
    auto c0 = lead_then_pe(gk, below(s.G, hid_col), s.Lv, s.G);
    auto sigma = [&](int l, int tiles, auto row) {
        const float* Wl = A + v.param_off[v.sigma_blk(l)];
        if (l == 0) sb.layer_rc(Wl, v.input_ch, tiles, kf + PE_KS, pad_each, row, in0);
        else sb.layer_rc(Wl, s.HD, tiles, s.KS, pad_each, row, hid_col);
    };
    for (int l = 0; l + 1 < s.NS; ++l) sigma(l, s.T, rows_upto(s.HD));
    sigma(s.NS - 1, 1, density_row);
    for (int t = 0; t < s.GT; ++t) sigma(s.NS - 1, 1, geo_rows(s.G, t));
    for (int l = 0; l < s.NC; ++l) {
        const bool last = l == s.NC - 1;
        const float* Wl = A + v.param_off[v.color_w_blk(l)];
        if (l == 0) sb.layer(Wl, last ? 3 : s.HD, s.G + s.ICV, last ? 1 : s.T, gk + PEV_KS, pad_each || last, c0);
        else sb.layer(Wl, last ? 3 : s.HD, s.HD, last ? 1 : s.T, s.KS, pad_each || last, hid_col);
    }
}

// A standard level in the table of k_voxel_mlp (kernel_voxel.hip).  Its own sequence: on the coarse level (1 + G <= 32) sigma and geo are
// ONE fused tile, which color_net.0 reads through fused_geo_col; the fine level's geo tiles are full
inline void voxel_layers_legacy(StreamBuilder& sb, const evd_voxel& v, const float* A) {
    const VoxDims s(v);
    const int HD = s.HD, G = s.G, T = s.T, KS = s.KS, gk = 1 + G <= 32 ? 1 : G / 16;
    const float *sigma_w0 = A + v.param_off[0], *sigma_w1 = A + v.param_off[1];
    sb.layer(sigma_w0, HD, v.input_ch, T, s.KF + PE_KS, false, lead_then_pe(s.KF, nat_col(s.FT), s.L, s.FT));
    if (1 + G <= 32) {
        sb.layer(sigma_w1, 1 + G, HD, 1, KS, false, hid_col);
        sb.layer(A + v.param_off[2], HD, G + s.ICV, T, gk + PEV_KS, false, lead_then_pe(gk, fused_geo_col(G), s.Lv, G));
    } else {
        sb.layer_rc(sigma_w1, HD, 1, KS, false, density_row, hid_col);
        sb.layer_rc(sigma_w1, HD, G / 32, KS, false, geo_rows(G), hid_col);
        sb.layer(A + v.param_off[2], HD, G + s.ICV, T, gk + PEV_KS, false, lead_then_pe(gk, below(G, hid_col), s.Lv, G));
    }
    sb.layer(A + v.param_off[4], HD, HD, T, KS, false, hid_col);
    sb.layer(A + v.param_off[6], 3, HD, 1, KS, true, hid_col);
}

// The compensated mode's table of the standard fine level (voxel_mlp_c_kernel.h VoxNetC): groups of two tiles, 64-input blocks
inline void voxel_layers_c(StreamBuilderC& sc, const evd_voxel& v, const float* A) {
    const VoxDims s(v);
    const int HD = s.HD, G = s.G, T = s.T, KS = s.KS;
    const float* sigma_w1 = A + v.param_off[1];
    auto sig_at = [=](int r, int c) -> const float* { return c < HD ? sigma_w1 + (size_t)r * HD + c : nullptr; };
    sc.arena = A;
    sc.layer(A + v.param_off[0], HD, v.input_ch, T, s.KF + PE_KS, 2, lead_then_pe(s.KF, nat_col(s.FT), s.L, s.FT));
    sc.layer_at(1, KS, 1, density_row, c_hid_col, sig_at);
    sc.layer_at(s.GT, KS, 2, geo_rows(G), c_hid_col, sig_at);
    sc.layer(A + v.param_off[2], HD, G + s.ICV, T, s.GK + PEV_KS, 2, lead_then_pe(s.GK, below(G, c_hid_col), s.Lv, G));
    sc.layer(A + v.param_off[4], HD, HD, T, KS, 2, c_hid_col);
    sc.layer(A + v.param_off[6], 3, HD, 1, KS, 1, c_hid_col);
}

// The W^T streams of a standard level's dgrad chain in mode prec (voxel_train_kernel.h)
inline int voxel_wt_streams(evd_voxel& v, int prec, const float* A) {
    const VoxDims s(v);
    const int HD = s.HD, G = s.G, T = s.T, KS = s.KS;
    const float *sigma_w0 = A + v.param_off[0], *sigma_w1 = A + v.param_off[1], *color_w0 = A + v.param_off[2], *color_w1 = A + v.param_off[4],
                *color_w2 = A + v.param_off[6];
    auto put = [&](int which, auto fill) { return put_wt(v.bwd[prec][which], prec, A, fill); };
    int rc = put(VBWD_C2, [&](StreamBuilder& b) { b.layer_transposed(color_w2, 3, HD, 0, HD, nullptr, 0, T, 1, true, nat_col(3)); });
    if (!rc) rc = put(VBWD_C1, [&](StreamBuilder& b) { b.layer_transposed(color_w1, HD, HD, 0, HD, nullptr, 0, T, KS, true, hid_col); });
    // [geo rows | direction-encoding rows] of color_net.0
    if (!rc) rc = put(VBWD_C0, [&](StreamBuilder& b) { enc_layer_wt(b, color_w0, G + s.ICV, G, G, s.Lv, 1, KS); });
    if (!rc) rc = put(VBWD_SIGGEO, [&](StreamBuilder& b) {      // the geo rows of sigma_net.1 in color_net.0's column order, then its density row
        b.layer_transposed(sigma_w1, 1 + G, HD, 0, HD, nullptr, 0, T, s.GK + 1, true, lead_then_one(s.GK, offset(1, below(G, hid_col)), 0));
    });
    // [feature rows | point-encoding rows] of sigma_net.0
    if (!rc) rc = put(VBWD_L0, [&](StreamBuilder& b) { enc_layer_wt(b, sigma_w0, v.input_ch, s.FT, s.FT, s.L, 2, KS); });
    return rc;
}

// wgrad index maps of a standard level (voxel_train.h)
inline std::vector<int> voxel_wgrad_maps(const evd_voxel& v) {
    const VoxDims s(v);
    std::vector<int> m(VMAP_TOTAL, -1);
    auto copy = [&](int to, int from, int n) { for (int i = 0; i < n; ++i) m[to + i] = m[from + i]; };
    fill_map(m, VMAP_HID, 256, below(s.HD, hid_col));
    fill_map(m, VMAP_FTS, 64, nat_col(s.FT));
    fill_map(m, VMAP_PE, 64, pe_at(s.L, s.FT));
    fill_map(m, VMAP_DIR, 32, pe_at(s.Lv, s.G));
    fill_map(m, VMAP_GEO_X, 128, below(s.G, hid_col));
    fill_map(m, VMAP_GEO_Y, 128, offset(1, below(s.G, hid_col)));
    fill_map(m, VMAP_COL, 3, nat_col(3));
    m[VMAP_SIG] = 0;
    copy(VMAP_F64_SG, VMAP_GEO_Y, 16); copy(VMAP_F64_SG + 16, VMAP_SIG, 16);
    copy(VMAP_F64_C0, VMAP_GEO_X, 32); copy(VMAP_F64_C0 + 32, VMAP_DIR, 32);
    copy(VMAP_F64_L0, VMAP_FTS, 32); copy(VMAP_F64_L0 + 32, VMAP_PE, 64);
    copy(VMAP_SG5, VMAP_GEO_Y, 128); copy(VMAP_SG5 + 128, VMAP_SIG, 32);
    return m;
}

}  // namespace evd
