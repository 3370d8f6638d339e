// The PDRF level of any depth, width and geo size (kernel_voxel_generic.hip): what its kernel and evd_voxel_create's stream builder share.
// reference: networks/pdrf/voxnerf.py:48-82 (the layer shapes), options.py:134-163 (the options that set them).
#pragma once

#include "nerf_mlp.h"
#include "voxel.h"

namespace evd {

constexpr int VG_MAX_LAYERS = 4;        // num_layers and num_layers_color: 1..4
constexpr int VG_GT = 4;                // geo tiles: geo_feat_dim <= 128
constexpr int VG_GK = 2 * VG_GT;        // geo k-steps of color_net.0's input, always all of them (absent tiles: zero)
constexpr int VG_KF = 4;                // feature k-steps of sigma_net.0's input, always all of them (FT <= 64; absent channels: zero)

struct VoxGenShape {
    int ns, nc;         // num_layers, num_layers_color
    int G, gt;          // geo_feat_dim and its 32-channel tiles
    int kf;             // FT / 16: feature k-steps read from the rows
};

// The STANDARD levels keep every stream and kernel they have (pipelined, resident, f16c, training); everything else evd_voxel_create accepts
// is a generic level
inline bool voxel_standard_shape(int num_layers, int num_layers_color, int HD, int G, int FT) {
    return num_layers == 2 && num_layers_color == 3 && ((HD == 64 && G == 15 && FT == 32) || (HD == 256 && G == 128 && FT == 64));
}

int voxel_mlp_generic_dispatch(int prec, int HD, const VoxMlpParams& p, const VoxGenShape& g, hipStream_t st);

// ---- training of a generic level, EVD_PREC_F16X3 (kernel_voxel_train_generic.hip), built like the generic NeRF path on the per-layer kernels of gen_rows.h
// The store: planes of float32 rows, nsp = nsamp rounded up to the 32-sample tile.  Offsets in floats.
constexpr int VG_FT_LD = 16 * VG_KF, VG_GEO_LD = 32 * VG_GT, VG_COL_LD = 32;
struct VoxGenStore {
    long nsp;
    int HD, NS, NC;
    __host__ __device__ VoxGenStore(long nsamp, int HD_, int NS_, int NC_) : nsp((nsamp + 31) / 32 * 32), HD(HD_), NS(NS_), NC(NC_) {}
    // what the forward writes
    __host__ __device__ long in() const { return 0; }                                      // [nsp, 8]: pts xyz, 0, viewdir xyz, 0
    __host__ __device__ long fts() const { return nsp * 8; }                               // [nsp, 64]: the sampled features, FT columns
    __host__ __device__ long hs(int l) const { return nsp * (8 + VG_FT_LD + (long)l * HD); }    // [nsp, HD]: ReLU output of sigma_net.l, l < NS - 1
    __host__ __device__ long geo() const { return hs(NS - 1); }                            // [nsp, 128]: sigma_net.(NS-1) rows 1..G, G columns
    __host__ __device__ long hc(int l) const { return geo() + nsp * (VG_GEO_LD + (long)l * HD); }   // [nsp, HD]: ReLU output of color_net.l, l < NC - 1
    __host__ __device__ long fwd_total() const { return hc(NC - 1); }
    // what the backward writes
    __host__ __device__ long g(int i) const { return fwd_total() + i * nsp * HD; }         // [nsp, HD] x 2: d loss / d pre-activation, ping-pong
    __host__ __device__ long dgeo() const { return g(2); }                                 // [nsp, 128]: d geo rows, zero from column G on
    __host__ __device__ long dcol() const { return dgeo() + nsp * VG_GEO_LD; }             // [nsp, 32]: d colour pre-activations, zero from column 3 on
    __host__ __device__ long enc(int i) const { return dcol() + nsp * VG_COL_LD + i * nsp * 64; }   // [nsp, 64] x 4: PE(pts), PE(dirs) and their gradients
    __host__ __device__ long total() const { return enc(4); }
};

int voxel_train_fwd_generic_dispatch(int HD, const VoxMlpParams& p, const VoxGenShape& g, hipStream_t st);

struct VoxGenBwdPlan {
    int HD, G, FT, NS, NC, L, Lv;
    const float* params;            // the handle's float32 parameters, canonical order
    const long* off;                // block offsets: sigma_net.l at [l], color_net.l.{weight,bias} at [NS + 2 l], [NS + 2 l + 1]
    const float *d_raw, *raw, *d_feature;   // [nsamp, 4] x 2, [nsamp, G] or null
    long nsamp;
    float *store, *partial;         // VoxGenStore, GEN_WS_FLOATS floats
    float *sigma_w[VG_MAX_LAYERS], *color_w[VG_MAX_LAYERS], *color_b[VG_MAX_LAYERS];     // gradients, null: not wanted
    int accumulate;
    float* d_fts; int d_fts_stride; // [nsamp, d_fts_stride] or null
    float *d_pts, *d_dirs;          // [nsamp, 3] or null
};
int run_voxel_backward_generic(const VoxGenBwdPlan& b, hipStream_t st);

}  // namespace evd
