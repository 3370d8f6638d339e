// The fragment arrangements of the packed weight streams, each stated ONCE (host code; included by the users of pack.h's builders):
// the layout contract of nerf_mlp.h between the packers (nerf_streams.h, voxel_streams.h, evd_awp_api.hip) and every MLP kernel.
//   column map  col(j, kk)  k-step j, position kk     -> input channel of the layer's weight matrix, -1 = zero padding
//   row map     row(t, r)   output tile t, row r      -> output row of the weight matrix, -1 = zero row
// A wrong map packs, trains and renders without an error and gives wrong numbers: every map below is what some kernel's fragments hold.
#pragma once

#include "mlp_pipe.h"
#include "pack.h"

namespace evd {

// ---- column maps
// a hidden block: the D fragments of the layer before, read as B fragments (nerf_mlp.h).  The compensated mode's: c_hid_col (pack.h)
constexpr int hid_col(int j, int kk) { return 16 * j + phi(kk); }
// an encoding of L frequencies in its own arrangement -> column of the reference's PE vector
constexpr int pe_col(int L, int j, int kk) { return pe_src_col(L, 8 * j + (kk & 7), kk >> 3); }
// channels in natural order (float32 rows loaded 16 per k-step; a 3-channel gradient fragment), absent beyond n
inline auto nat_col(int n) { return [n](int j, int kk) { return 16 * j + kk < n ? 16 * j + kk : -1; }; }
// col, with the channels from n on absent
template <class Col> auto below(int n, Col col) { return [=](int j, int kk) { const int c = col(j, kk); return c < n ? c : -1; }; }
// col, moved behind `by` other columns (rows) of the matrix
template <class Col> auto offset(int by, Col col) { return [=](int j, int kk) { const int c = col(j, kk); return c < 0 ? -1 : by + c; }; }
inline auto pe_at(int L, int col0) { return offset(col0, [L](int j, int kk) { return pe_col(L, j, kk); }); }
// cat([block, encoding]): n leading k-steps from lead(j, kk), then the encoding of L frequencies behind the block's col0 columns
template <class Lead> auto lead_then_pe(int n, Lead lead, int L, int col0) {
    return [=, pe = pe_at(L, col0)](int j, int kk) { return j < n ? lead(j, kk) : pe(j - n, kk); };
}
// n leading k-steps from lead(j, kk), then one k-step whose position 0 is column `col` (a W^T layer with one more output appended)
template <class Lead> auto lead_then_one(int n, Lead lead, int col) { return [=](int j, int kk) { return j < n ? lead(j, kk) : (kk == 0 ? col : -1); }; }
// The standard coarse level's color_net.0 in the table of k_voxel_mlp: its geo k-step reads the FUSED sigma + geo tile (channel c at row 1 + c)
inline auto fused_geo_col(int G) { return [G](int j, int kk) { const int row = hid_col(j, kk); return row >= 1 && row <= G ? row - 1 : -1; }; }
// The NeRF skip layer cat([PE(pts), h]) (networks/nerf.py:137-138): the encoding's PE_KS k-steps after `at` hidden k-steps (0: encoding
// first), the hidden channels behind the encoding's IC columns
template <class Hid> auto wide_col(int at, int L, int IC, Hid hid) {
    return [=](int j, int kk) {
        if (j >= at && j < at + PE_KS) return pe_col(L, j - at, kk);
        return IC + hid(j < at ? j : j - PE_KS, kk);
    };
}

// ---- row maps
// natural rows up to out_dim, from tile t0 on (what pack.h's layer() uses from tile 0)
inline auto rows_upto(int out_dim, int t0 = 0) { return [=](int t, int r) { const int c = 32 * (t0 + t) + r; return c < out_dim ? c : -1; }; }
// sigma_net's last layer [1 + G, *]: the density row alone in a tile; the geo rows in zero-padded 32-row tiles, from tile t0 on
constexpr int density_row(int, int r) { return r == 0 ? 0 : -1; }
inline auto geo_rows(int G, int t0 = 0) { return [=](int t, int r) { const int c = 32 * (t0 + t) + r; return c < G ? 1 + c : -1; }; }
// rows of an encoding appended to a W^T layer: output row idx <-> encoding column, so that the output fragments come out in the
// encoding's own arrangement (fragment j, position kk <-> pe_col(L, j, kk))
constexpr int enc_row(int L, int idx) { return pe_col(L, idx / 16, phi_inv(idx % 16)); }

// ---- wgrad index maps (nerf_train.h MAP_*, voxel_train.h VMAP_*, awp_embed.h AMAP_*): entry i <-> fragment j = i / 16, position kk = i % 16
template <class Col> void fill_map(std::vector<int>& m, int at, int n, Col col) { for (int i = 0; i < n; ++i) m[at + i] = col(i / 16, i % 16); }

// ---- the builders of the pipelined kernels' streams: 16 KiB chunks, every element's source recorded for the device re-pack
inline StreamBuilder pipe_builder(int prec, const float* arena, int group = 1) {
    StreamBuilder sb(prec, PIPE_CB);
    sb.arena = arena; sb.group = group;
    return sb;
}
// one W^T stream of a dgrad chain (single-tile groups): fill(builder) appends its layer
template <class Fill> int put_wt(PackedStream& dst, int prec, const float* arena, Fill fill) {
    StreamBuilder sb = pipe_builder(prec, arena);
    fill(sb);
    return dst.upload(sb);
}
// The W^T layer of a first layer Wm [*, in_dim] for the gradient w.r.t. its input cat([lead channels, encoding of L frequencies at column
// col0]): ceil(lead / 32) tiles of the channels' rows (lead 0: none), then enc_tiles tiles of the encoding's rows (enc_row); the
// columns are the layer's outputs in hidden order
inline void enc_layer_wt(StreamBuilder& b, const float* Wm, int in_dim, int lead, int col0, int L, int enc_tiles, int ksteps) {
    const int LT = (lead + 31) / 32;
    b.layer_at(LT + enc_tiles, ksteps, true,
               [=](int t, int r) {
                   if (t < LT) return 32 * t + r < lead ? 32 * t + r : -1;
                   const int c = enc_row(L, 32 * (t - LT) + r);
                   return c < 0 ? -1 : col0 + c;
               },
               hid_col, [=](int r, int c) { return Wm + (size_t)c * in_dim + r; });
}

// ---- the parameter arena: the blocks (host source or null = zeros, size) in canonical order -> off[0..n] (off[n] = the total) and the
// host copy every packed element's source index refers to
struct ParamBlock { const float* src; long size; };
inline std::vector<float> build_arena(const ParamBlock* blk, int n, long* off) {
    long total = 0;
    for (int i = 0; i < n; ++i) { off[i] = total; total += blk[i].size; }
    off[n] = total;
    std::vector<float> arena((size_t)total, 0.f);
    for (int i = 0; i < n; ++i)
        if (blk[i].src) memcpy(arena.data() + off[i], blk[i].src, blk[i].size * sizeof(float));
    return arena;
}

// ---- the bias image: one 32-float row block per output tile in stream order, and per value its source in the arena (-1: zero) for the
// re-pack (k_gather_f32)
struct BiasImage {
    const float* arena;
    const long* off;                // the handle's param_off
    std::vector<float> b;
    std::vector<int32_t> src;       // what the handle keeps as bias_src
    BiasImage(const float* arena_, const long* param_off, int zeros = 0) : arena(arena_), off(param_off), b(zeros, 0.f), src(zeros, -1) {}
    void push(int block, int out_dim, int tiles) {
        for (int i = 0; i < tiles * 32; ++i) {
            b.push_back(i < out_dim ? arena[off[block] + i] : 0.f);
            src.push_back(i < out_dim ? (int32_t)(off[block] + i) : -1);
        }
    }
    int upload(DevBuf& bias, DevBuf& bias_src) const {
        const int rc = bias.upload(b.data(), b.size() * sizeof(float));
        return rc ? rc : bias_src.upload(src.data(), src.size() * sizeof(int32_t));
    }
};

}  // namespace evd
