// The opaque evd_voxel handle of include/evdnerf.h and what the units of its C ABI share: evd_voxel_api.hip (create, parameters),
// evd_voxel_render_api.hip (inference, c2f render), evd_voxel_train_api.hip (network training), evd_voxel_grids_api.hip (the grids as parameters).
#pragma once

#include "evd_common.h"
#include "pack.h"
#include "voxel.h"
#include "voxel_generic.h"
#include "voxel_train.h"

// the PDRF level networks keep packed streams for the first four arithmetic modes; EVD_PREC_F16C (compensated float16) has its own
// stream (pipe_c) on the standard fine level; every other level runs EVD_PREC_F16X3 next to it
#define EVD_VOX_NUM_PREC EVD_PREC_F16C

struct evd_voxel {
    typedef evd::DevBuf DevBuf;
    typedef evd::PackedStream PackedStream;
    int num_layers, hidden_dim, geo, num_layers_color, input_ch, ft_dim, app_dim;
    int n_comp[3], grid[3], app_act, rgb_act, sigma_act, composite_feature;
    float aabb[6], rmnear;
    int multires = evd::PE_L, multires_views = evd::PE_LV;
    DevBuf plane[3], line[3], plane_h[3], line_h[3], basis, bias, bias_src, tv_acc, wmaps;
    // fwd: the level's network in the layer table of voxel_mlp_kernel.h, ONE stream per mode of a standard level (is_train_prec): the
    // render pass and the training forward both read it.  stream: the generic kernel's layout (kernel_voxel.hip), built only where
    // voxel_level_forward can select it (has_generic_stream).  bwd: the W^T streams of the training backward.  (voxel_streams.h)
    PackedStream stream[EVD_VOX_NUM_PREC], fwd[EVD_VOX_NUM_PREC], bwd[EVD_VOX_NUM_PREC][evd::VBWD_NSTREAMS];
    int nchunks[EVD_VOX_NUM_PREC], fwd_chunks[EVD_VOX_NUM_PREC];
    mutable evd::PackedStreamC pipe_c; // compensated float16 mode (voxel_mlp_c_kernel.h): float16 + fp6 fragments and row scales; fine level only
    int pipe_c_chunks = 0;
    // its re-pack after evd_voxel_load_params is LAZY (a training loop re-loads every iteration and never renders in this mode): the new
    // parameter values are kept in `arena_dev` (one stream-ordered device copy) and re-packed by the first f16c launch that follows
    mutable DevBuf arena_dev;
    mutable bool pipe_c_stale = false;
    DevBuf cnet;                  // composite_feature levels: color_net.{0,1,2}.{weight,bias} as float32 in the reference layouts (k_color_rows)
    // sigma_net.0 .. num_layers-1, then color_net.l.{weight,bias} in the parameter arena, [nblk] = total (a standard level: 8 blocks)
    long param_off[evd::VG_MAX_LAYERS + 2 * evd::VG_MAX_LAYERS + 1];
    int nblk;
    // a level of any other shape than the two standard ones (voxel_generic.h): `stream` holds the layout of kernel_voxel_generic.hip in every
    // mode, fwd / bwd / pipe_c stay empty; params_f32 is the float32 copy of the parameters its training backward reads in place
    bool generic = false;
    DevBuf params_f32;
    int sigma_blk(int l) const { return l; }
    int color_w_blk(int l) const { return num_layers + 2 * l; }
    int color_b_blk(int l) const { return num_layers + 2 * l + 1; }
    evd::GridParams gp;
    evd::RepackBatch batch;       // table of every fragment stream, for the one-launch re-pack of evd_voxel_load_params
    mutable evd::SideStream side; // backward entry: wgrad side stream of THIS handle (created on first use)
};

namespace evd {

static const int kMat0[3] = {0, 0, 1}, kMat1[3] = {1, 2, 2}, kVec[3] = {2, 1, 0};

// Where voxel_level_forward can take k_voxel_mlp on a STANDARD level, i.e. which levels and modes need its `stream`: a mode or an encoding
// without a pipelined stream (EVD_PREC_F32, non-standard multires / multires_views), and the standard coarse level (64/15/32) in every mode:
// for per-sample feature rows (also the geo rows of a composite_feature level) it has no other kernel.  The standard fine level's pipelined
// kernels write those rows themselves.
inline bool std_coarse(const evd_voxel* v) { return !v->generic && v->hidden_dim == 64; }
inline bool has_generic_stream(bool piped, bool coarse) { return !piped || coarse; }

// the shape a generic level's kernels are dispatched on
inline VoxGenShape vox_gen_shape(const evd_voxel* v) { return VoxGenShape{v->num_layers, v->num_layers_color, v->geo, (v->geo + 31) / 32, v->ft_dim / 16}; }

// sampling inside the c2f render and its backward: the half-precision arithmetic modes read the float16 copies of the grids
inline bool grids_half_for(const evd_voxel* v, int precision) {
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

// EVD_PREC_F16C trains on the single-product float16 store and backward behind a compensated forward: the level's f16c kernel where
// that is built (fine level), else the split-float16 forward writing the float16 store (coarse level)
// EVD_PREC_F16M: the split-float16 forward on every level, same store and backward
inline bool vox_train_built(const evd_voxel* v, int prec) {
    if (v->generic) return prec == EVD_PREC_F16X3;      // kernel_voxel_train_generic.hip; the other modes' training kernels are the standard levels'
    if (prec == EVD_PREC_F16C) return v->fwd_chunks[EVD_PREC_F16] > 0 && (v->pipe_c_chunks > 0 || v->fwd_chunks[EVD_PREC_F16X3] > 0);
    if (prec == EVD_PREC_F16M) return v->fwd_chunks[EVD_PREC_F16] > 0 && v->fwd_chunks[EVD_PREC_F16X3] > 0;
    return prec >= 0 && prec < EVD_VOX_NUM_PREC && v->fwd_chunks[prec] > 0;
}
inline int vox_store_prec(int prec) { return (prec == EVD_PREC_F16C || prec == EVD_PREC_F16M) ? EVD_PREC_F16 : prec; }

// what the inference pass and the training forward of a level fill alike (the stream is chosen later, with the kernel)
inline VoxMlpParams vox_mlp_params(const evd_voxel* v, const float* pts, const float* viewdirs, int vd_stride, const float* fts, int ft_stride,
                                   long R, int S, float* raw, float* feature, char* act) {
    VoxMlpParams p{};
    p.pts = pts; p.viewdirs = viewdirs; p.fts = fts; p.nsamp = R * (long)S; p.S = S; p.vd_stride = vd_stride; p.ft_stride = ft_stride;
    p.bias = (const float*)v->bias.p; p.nbias = (int)(v->bias.bytes / sizeof(float)); p.raw = raw; p.feature = feature; p.act = act;
    return p;
}

// the compensated mode's stream into p, re-packed first if evd_voxel_load_params has run since its last use
inline int use_pipe_c(const evd_voxel* v, VoxMlpParams& p, hipStream_t st) {
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

}  // namespace evd
