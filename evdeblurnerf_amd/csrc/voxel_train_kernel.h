// Backward of one PDRF level's sigma / colour networks (reference: autograd of VoxelNeRFBase.forward, networks/pdrf/voxnerf.py:210-254)
// on the dgrad / wgrad kernels of nerf_train_kernel.h; slots: voxel_mlp_kernel.h VStore.
//
//   raw = (sigma, sigmoid(colour)):  d colour_pre = d raw_c . s (1 - s) is folded into the gradient fragments
//   C2^T -> d c1 . [c1 > 0];  C1^T -> d c0 . [c0 > 0];  C0^T (geo rows) -> d geo;  [Geo^T | Sigma^T] -> d hid . [hid > 0];
//   L0^T (feature rows) -> d fts, written out as float32 rows for the tri-plane scatter (kernel_voxel_sample_bwd.hip k_voxel_sample_bwd)
#pragma once

#include "nerf_train_kernel.h"
#include "voxel_mlp_kernel.h"
#include "voxel_train.h"
#include "voxel_bwd_fused64.h"

namespace evd {

template <int PREC>
__global__ __launch_bounds__(256) void k_voxel_grad_frags(const float* __restrict__ d_raw, const float* __restrict__ raw, long nsamp,
                                                          const unsigned* __restrict__ maxbits, char* __restrict__ store, long tiles,
                                                          long tile_bytes, int g_col, int g_sig) {
    typedef POps<PREC> O;
    typedef typename O::B B;
    pipe_fp16_saturate<PREC>();
    const long idx = (long)blockIdx.x * 256 + threadIdx.x, tile = idx >> 6;
    if (tile >= tiles) return;
    const int lane = idx & 63, n = lane & 31, h = lane >> 5;
    const long smp = tile * 32 + n;
    const float s = grad_scale(*maxbits, false);
    f32x4 g = {0.f, 0.f, 0.f, 0.f};
    if (h == 0 && smp < nsamp) {
        g = *reinterpret_cast<const f32x4*>(d_raw + smp * 4);
        const f32x4 r = *reinterpret_cast<const f32x4*>(raw + smp * 4);
#pragma unroll
        for (int c = 1; c < 4; ++c) g[c] = g[c] * r[c] * (1.f - r[c]);         // through torch.sigmoid (voxnerf.py:252)
    }
    B col, sg;
    O::zero(col);
    O::zero(sg);
    O::template set_pair<false>(col, 0, g[1] * s, g[2] * s);
    O::template set_pair<false>(col, 1, g[3] * s, 0.f);
    O::template set_pair<false>(sg, 0, g[0] * s, 0.f);
    constexpr int FB = frag_bytes(PREC);
    char* a = store + tile * tile_bytes + lane * 16;
    act_store<FB>(a, g_col, col);
    act_store<FB>(a, g_sig, sg);
}

// gradient fragments of the input features -> float32 rows [n, FT] (loss scale removed): fragment j, position kk of the dgrad
// output <-> feature 16 j + phi(kk)
template <int PREC>
__global__ __launch_bounds__(256) void k_frags_to_rows(const char* __restrict__ store, long tile_bytes, int slot, int nfrag, long nsamp,
                                                       const unsigned* __restrict__ maxbits, float* __restrict__ rows, int stride) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long tile = idx / (64 * nfrag);
    const int j = (int)((idx / 64) % nfrag), lane = idx & 63, n = lane & 31, h = lane >> 5;
    const long smp = tile * 32 + n;
    if (smp >= nsamp) return;
    float fv[8];
    frag_values<PREC>(store + tile * tile_bytes + lane * 16, slot + j, fv);
    const float inv = grad_scale(*maxbits, true);
#pragma unroll
    for (int e = 0; e < 8; ++e) rows[smp * (long)stride + 16 * j + phi(8 * h + e)] = fv[e] * inv;
}
template <int PREC> int BwdChain::frags_to_rows(int slot, int nfrag, float* rows, int stride) const {
    hipLaunchKernelGGL((k_frags_to_rows<PREC>), dim3((unsigned)cdiv(tiles * 64 * nfrag, 256L)), dim3(256), 0, st, (const char*)store, tile_bytes, slot, nfrag, nsamp,
                       maxbits, rows, stride);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

// activation fragments -> float32 rows [n, nch] (no scale): the geo rows of the 64-wide level, whose training forward writes no rows
// itself (voxel_mlp_kernel.h: rows leave the pipelined kernel 32 channels at a time) -- in the half-precision modes they are the rounded
// values the level's colour layer consumed
template <int PREC>
__global__ __launch_bounds__(256) void k_act_frags_to_rows(const char* __restrict__ store, long tile_bytes, int slot, int nfrag, long nsamp,
                                                           float* __restrict__ rows, int nch) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long tile = idx / (64 * nfrag);
    const int j = (int)((idx / 64) % nfrag), lane = idx & 63, n = lane & 31, h = lane >> 5;
    const long smp = tile * 32 + n;
    if (smp >= nsamp) return;
    float fv[8];
    frag_values<PREC>(store + tile * tile_bytes + lane * 16, slot + j, fv);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int ch = 16 * j + phi(8 * h + e);
        if (ch < nch) rows[smp * (long)nch + ch] = fv[e];
    }
}
// the geo rows of a training forward that kept its activations in p.act, into p.feature
template <int PREC, int HD, int G, int FT> static int voxel_geo_rows_from_store(const VoxMlpParams& p, hipStream_t st) {
    typedef VStore<HD, G, FT> VS;
    constexpr int NF = (G + 15) / 16;
    const long tiles = cdiv(p.nsamp, 256L) * 8;
    hipLaunchKernelGGL((k_act_frags_to_rows<PREC>), dim3((unsigned)cdiv(tiles * 64 * NF, 256L)), dim3(256), 0, st, (const char*)p.act, VS::tile_bytes(PREC), VS::GEO, NF,
                       p.nsamp, p.feature, G);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}
// the 64-wide level's training forward with the geo rows wanted (a composite_feature level composites them per ray)
template <int PREC> static int launch_voxel_train_fwd64_rows(const VoxMlpParams& p, hipStream_t st) {
    VoxMlpParams q = p;
    q.feature = nullptr;
    const int rc = launch_voxel_train_fwd<PREC, 64, 15, 32>(q, st);
    return rc ? rc : voxel_geo_rows_from_store<PREC, 64, 15, 32>(p, st);
}

// float32 gradient rows (the per-sample geo features' gradient, from the AWP consumer or the feature composite of a composite_feature
// level) added into gradient fragments: fragment j, position kk <-> channel 16 j + phi(kk), channels < nch (the 64-wide level's 15 geo
// channels leave one position of their fragment as it is); rows are scaled by the loss scale first
template <int PREC>
__global__ __launch_bounds__(256) void k_rows_add_to_frags(char* __restrict__ store, long tile_bytes, int slot, int nfrag, long nsamp,
                                                           const unsigned* __restrict__ maxbits, const float* __restrict__ rows, int stride, int nch) {
    typedef POps<PREC> O;
    pipe_fp16_saturate<PREC>();
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long tile = idx / (64 * nfrag);
    const int j = (int)((idx / 64) % nfrag), lane = idx & 63, n = lane & 31, h = lane >> 5;
    const long smp = tile * 32 + n;
    if (smp >= nsamp) return;
    char* a = store + tile * tile_bytes + lane * 16;
    const float s = grad_scale(*maxbits, false);
    float v[8];
    frag_values<PREC>(a, slot + j, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int ch = 16 * j + phi(8 * h + e);
        if (ch < nch) v[e] += rows[smp * (long)stride + ch] * s;
    }
    typename O::B b;
#pragma unroll
    for (int e = 0; e < 4; ++e) O::template set_pair<false>(b, e, v[2 * e], v[2 * e + 1]);
    act_store<frag_bytes(PREC)>(a, slot + j, b);
}

// *dst = max(*dst, *src) on float bits (both non-negative): the loss scale also covers a gradient that arrives as fragments
static __global__ void k_max_word(unsigned* __restrict__ dst, const unsigned* __restrict__ src) { atomicMax(dst, *src); }

// gradient fragments of ANOTHER store (the AWP embedding's d geo, awp_embed.h: its own loss-scale word) added into this level's
template <int PREC>
__global__ __launch_bounds__(256) void k_frags_add_scaled(char* __restrict__ store, long tile_bytes, int slot, const char* __restrict__ src, long src_tile_bytes,
                                                          int src_slot, int nfrag, long tiles, const unsigned* __restrict__ maxbits,
                                                          const unsigned* __restrict__ src_maxbits) {
    typedef POps<PREC> O;
    pipe_fp16_saturate<PREC>();
    const long idx = (long)blockIdx.x * 256 + threadIdx.x, tile = idx / (64 * nfrag);
    if (tile >= tiles) return;
    const int j = (int)((idx / 64) % nfrag), lane = idx & 63;
    char* a = store + tile * tile_bytes + lane * 16;
    static_assert(is_half_prec(PREC), "the AWP embedding's store is half precision: both stores share one fragment format");
    const float s = grad_scale(*maxbits, false) * grad_scale(*src_maxbits, true);
    float v[8], g[8];
    frag_values<PREC>(a, slot + j, v);
    frag_values<PREC>(src + tile * src_tile_bytes + lane * 16, src_slot + j, g);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = fmaf(g[e], s, v[e]);
    typename O::B b;
#pragma unroll
    for (int e = 0; e < 4; ++e) O::template set_pair<false>(b, e, v[2 * e], v[2 * e + 1]);
    act_store(a, slot + j, b);
}

// ---- the backward of one level -----------------------------------------------------------------------------------------------
// the loss-scale word: the maximum over every gradient that enters the level
static int voxel_backward_scale(const VoxBwdPlan& b, int G, hipStream_t st) {
    EVD_HIP(hipMemsetAsync(b.maxbits, 0, sizeof(unsigned), st));
    hipLaunchKernelGGL(k_absmax, dim3(512), dim3(256), 0, st, b.d_raw, b.nsamp * 4, b.maxbits);
    EVD_LAUNCH_CHECK();
    if (b.d_feature) {          // the loss scale covers both incoming gradients
        hipLaunchKernelGGL(k_absmax, dim3(512), dim3(256), 0, st, b.d_feature, b.nsamp * G, b.maxbits);
        EVD_LAUNCH_CHECK();
    }
    if (b.awp_store) {          // ... and the d geo fragments of the AWP embedding's backward (true-unit maximum in its trailer)
        hipLaunchKernelGGL(k_max_word, dim3(1), dim3(1), 0, st, b.maxbits, b.awp_words + 1);
        EVD_LAUNCH_CHECK();
    }
    return EVD_OK;
}

// d fts leave the kernel that forms them as the float32 rows the scatter reads when they can be written with 16-byte stores
// (EVD_BWD_ROWS=0: fragments + k_frags_to_rows)
static bool voxel_rows_direct(const VoxBwdPlan& b) { return bwd_switches().rows && b.d_fts && b.d_fts_stride % 4 == 0 && ((uintptr_t)b.d_fts & 15) == 0; }

// The gradients of the level's inputs from their gradient fragments: d dirs through PE(dirs), d fts as rows, d pts through PE(pts).
// `which`: the ones whose fragments are complete at the point of the call.
enum { VOUT_DIRS = 1, VOUT_FTS = 2, VOUT_PTS = 4 };
template <int PREC, class VS, int FT> static int voxel_backward_inputs(const BwdChain& c, const VoxBwdPlan& b, int which) {
    int rc;
    if ((which & VOUT_DIRS) && b.d_dirs && (rc = c.template pe_bwd<PREC, PE_LV, PEV_KS>(VS::D_DIRPE, b.viewdirs, b.vd_stride, b.S, b.d_dirs, 0))) return rc;
    if ((which & VOUT_FTS) && b.d_fts && (rc = c.template frags_to_rows<PREC>(VS::D_FTS, FT / 16, b.d_fts, b.d_fts_stride))) return rc;
    if ((which & VOUT_PTS) && b.d_pts && (rc = c.template pe_bwd<PREC, PE_L, PE_KS>(VS::D_PE, b.pts, 3, 1, b.d_pts, 0))) return rc;
    return EVD_OK;
}

// The 64-wide level: the whole chain in one launch, the tile's gradient resident in registers (voxel_bwd_fused64.h), then the reduces of
// its partial blocks
template <int PREC> static int voxel_backward_fused64(const BwdChain& c, const VoxBwdPlan& b) {
    constexpr int HD = 64, G = 15, FT = 32, IC = 3 * (1 + 2 * PE_L), ICV = 3 * (1 + 2 * PE_LV);
    typedef VStore<HD, G, FT> VS;
    hipStream_t st = c.st;
    const int blocks = (int)(cdiv(b.tiles, 4L) < 256 ? cdiv(b.tiles, 4L) : 256);
    VoxBwdFusedParams fp;
    fp.d_raw = b.d_raw; fp.raw = b.raw; fp.nsamp = b.nsamp; fp.tiles = b.tiles; fp.store = b.store; fp.maxbits = b.maxbits; fp.partial = b.partial;
    for (int k = 0; k < VBWD_NSTREAMS; ++k) fp.wt[k] = b.wt[k];
    const bool rows_direct = voxel_rows_direct(b);
    fp.d_fts = rows_direct ? b.d_fts : nullptr; fp.d_fts_stride = b.d_fts_stride;
    EVD_SET_MAX_LDS((&k_voxel_bwd_fused64<PREC>), (size_t)f64::LDS_BYTES);
    hipLaunchKernelGGL((k_voxel_bwd_fused64<PREC>), dim3((unsigned)blocks), dim3(256), (size_t)f64::LDS_BYTES, st, fp);
    EVD_LAUNCH_CHECK();
    const VoxBwdGrads& g = b.grads;
    WreduceJobs jobs;
    auto job = [&](int i, int a0, int RT, int CT, bool bias, int ymap, int xmap, float* dW, int ld, float* db) {
        WreduceParams& q = jobs.j[i];
        q.partial = b.partial + (long)a0 * 1024; q.nparts = blocks; q.RT = dW ? RT : 0; q.CT = CT; q.NC = CT + (bias ? 1 : 0);
        q.rowmap = b.maps + ymap; q.colmap = b.maps + xmap; q.dW = dW; q.ld = ld; q.db = bias ? db : nullptr; q.maxbits = b.maxbits;
        q.accum = b.accumulate; q.part_stride = (long)f64::NBLK * 1024;
    };
    job(0, f64::A_C2, 1, 2, false, VMAP_COL, VMAP_HID, g.color_w[2], HD, nullptr);
    job(1, f64::A_C1, 2, 2, false, VMAP_HID, VMAP_HID, g.color_w[1], HD, nullptr);
    job(2, f64::A_C0, 2, 2, false, VMAP_HID, VMAP_F64_C0, g.color_w[0], G + ICV, nullptr);
    job(3, f64::A_SG, 1, 2, false, VMAP_F64_SG, VMAP_HID, g.sigma_w[1], HD, nullptr);
    job(4, f64::A_L0, 2, 3, false, VMAP_HID, VMAP_F64_L0, g.sigma_w[0], FT + IC, nullptr);
    hipLaunchKernelGGL(k_wgrad_reduce_jobs, dim3(2 * 3 * 4, WREDUCE_MAX_JOBS), dim3(256), 0, st, jobs);
    EVD_LAUNCH_CHECK();
    if (g.color_b[0] || g.color_b[1] || g.color_b[2]) {        // the shared bias block (columns: colour_net.2, .1 x 2 row tiles, .0 x 2)
        BiasColsParams bp;
        bp.partial = b.partial + (long)f64::A_BIAS * 1024; bp.nparts = blocks; bp.part_stride = (long)f64::NBLK * 1024; bp.ncols = 5;
        bp.rowmap[f64::B_C2] = b.maps + VMAP_COL; bp.db[f64::B_C2] = g.color_b[2];
        for (int yb = 0; yb < 2; ++yb) {
            bp.rowmap[f64::B_C1 + yb] = b.maps + VMAP_HID + 32 * yb; bp.db[f64::B_C1 + yb] = g.color_b[1];
            bp.rowmap[f64::B_C0 + yb] = b.maps + VMAP_HID + 32 * yb; bp.db[f64::B_C0 + yb] = g.color_b[0];
        }
        bp.maxbits = b.maxbits; bp.accum = b.accumulate;
        hipLaunchKernelGGL(k_bias_cols_reduce, dim3(5 * 32 / 4), dim3(256), 0, st, bp);
        EVD_LAUNCH_CHECK();
    }
    return voxel_backward_inputs<PREC, VS, FT>(c, b, VOUT_DIRS | (rows_direct ? 0 : VOUT_FTS) | VOUT_PTS);
}

// The per-layer sequence.  The 256-wide layers of the fine level run wgrad(l) and dgrad(l) in one launch in the half-precision modes
// (FUSABLE; nerf_bwd_fused.h k_wgrad_dgrad) when the layer's weight gradient is wanted; every other layer issues its wgrad before the
// dgrad that reads the same arrays (BwdChain::wgrad).
template <int PREC, int HD, int G, int FT> static int voxel_backward_layers(const BwdChain& c, const VoxBwdPlan& b) {
    typedef VStore<HD, G, FT> VS;
    constexpr int T = HD / 32, KS = HD / 16, KF = FT / 16, GT = VS::GT, FTT = (FT + 31) / 32, IC = 3 * (1 + 2 * PE_L), ICV = 3 * (1 + 2 * PE_LV);
    constexpr bool FUSABLE = is_half_prec(PREC) && T == 8;
    hipStream_t st = c.st;
    const BwdSwitches& sw = bwd_switches();
    const VoxBwdGrads& g = b.grads;
    const int wb = c.tile_grid();
    auto dgrad = [&](int stream, int in_slot, int extra_slot, int mask_slot, int out_slot) { return c.dgrad_params(b.wt[stream], in_slot, extra_slot, mask_slot, out_slot); };
    int rc;
    hipLaunchKernelGGL((k_voxel_grad_frags<PREC>), dim3((unsigned)cdiv(b.tiles * 64, 256L)), dim3(256), 0, st, b.d_raw, b.raw, b.nsamp, b.maxbits, b.store,
                       b.tiles, VS::tile_bytes(PREC), VS::G_COL, VS::G_SIG);
    EVD_LAUNCH_CHECK();
    // color_net.2 (+ sigmoid, folded into the gradient fragment)
    if ((rc = c.wgrad(launch_wgrad<PREC, 1, T, true>, wb, 1, T, g.color_b[2] != nullptr, VS::G_COL, VS::C1, VMAP_COL, VMAP_HID, g.color_w[2], HD, g.color_b[2]))) return rc;
    // color_net.1; in the fused form d c1 = (W2^T d colour) . [c1 > 0] is formed inside the launch from the pair [G_COL | M_C1]
    // (k_wgrad_dgrad YGEN: color_net.2's dgrad launch and the D_C1 round trip are gone; EVD_BWD_YGEN=0: the separate launch)
    const bool c1_fused = FUSABLE && g.color_w[1], ygen = c1_fused && sw.ygen;
    static_assert(VS::M_C1 == VS::G_COL + 1, "the formed gradient's two inputs are one fragment pair");
    if (!ygen && (rc = launch_dgrad<PREC, 1, T, 1, false, 2>(dgrad(VBWD_C2, VS::G_COL, -1, VS::M_C1, VS::D_C1), b.tiles, st))) return rc;
    if constexpr (FUSABLE) {
        if (c1_fused) {
            FusedExtra x;
            x.mask_slot = VS::M_C0;
            x.ygen_wt = ygen ? b.wt[VBWD_C2] : nullptr;
            rc = ygen ? c.fused(launch_wgrad_dgrad<PREC, 8, 8, 1, 8, 16, true>, 8, g.color_b[1] != nullptr, VS::G_COL, VS::C1 - KS, VMAP_HID, VMAP_HID, g.color_w[1], HD, g.color_b[1],
                                b.wt[VBWD_C1], VS::D_C0, x)
                      : c.fused(launch_wgrad_dgrad<PREC, 8, 8, 1>, 8, g.color_b[1] != nullptr, VS::D_C1, VS::C1 - KS, VMAP_HID, VMAP_HID, g.color_w[1], HD, g.color_b[1],
                                b.wt[VBWD_C1], VS::D_C0, x);
            if (rc) return rc;
        }
    }
    if (!c1_fused) {
        if ((rc = c.wgrad(launch_wgrad<PREC, T, T, false>, wb, T, T, g.color_b[1] != nullptr, VS::D_C1, VS::C1 - KS, VMAP_HID, VMAP_HID, g.color_w[1], HD, g.color_b[1]))) return rc;
        if ((rc = launch_dgrad<PREC, KS, T, KS, false, 2>(dgrad(VBWD_C1, VS::D_C1, -1, VS::M_C0, VS::D_C0), b.tiles, st))) return rc;
    }
    // color_net.0 on cat([geo, PE(dirs)])
    bool c0_fused = false;
    if constexpr (FUSABLE && G == 32 * GT) {
        if (g.color_w[0]) {     // wgrad + dgrad in one launch: d c0 read once; writes d geo | d PE(dirs) (no ReLU on geo)
            static_assert(VS::D_DIRPE == VS::D_GEO + 2 * GT, "d PE(dirs) behind d geo");
            // the geo and the direction-encoding columns are ONE operand of GT + 1 tiles
            static_assert(VS::DIRPE == VS::GEO + 2 * GT && VMAP_DIR == VMAP_GEO_X + 128 && (G == 128), "adjacent fragments and column maps");
            if ((rc = c.fused(launch_wgrad_dgrad<PREC, GT + 1, GT + 1, 0>, GT + 1, g.color_b[0] != nullptr, VS::D_C0, VS::GEO, VMAP_HID, VMAP_GEO_X, g.color_w[0], G + ICV, g.color_b[0],
                              b.wt[VBWD_C0], VS::D_GEO))) return rc;
            c0_fused = true;
        }                       // (not wanted: no wgrad, the dgrad below)
    } else {
        if ((rc = c.wgrad(launch_wgrad<PREC, T, GT, false>, wb, T, GT, g.color_b[0] != nullptr, VS::D_C0, VS::GEO, VMAP_HID, VMAP_GEO_X, g.color_w[0], G + ICV, g.color_b[0]))) return rc;
        if ((rc = c.wgrad(launch_wgrad<PREC, T, 1, false>, wb, T, 1, false, VS::D_C0, VS::DIRPE, VMAP_HID, VMAP_DIR, g.color_w[0], G + ICV, nullptr))) return rc;
    }
    if (!c0_fused && (rc = launch_dgrad<PREC, KS, GT + 1, KS, false, 0>(dgrad(VBWD_C0, VS::D_C0, -1, -1, VS::D_GEO), b.tiles, st))) return rc;   // d geo | d PE(dirs)
    if (b.d_feature) {          // + the gradient of the geo features as an output of the level (voxnerf.py:221, consumed by AWP)
        constexpr int NF = (G + 15) / 16;
        hipLaunchKernelGGL((k_rows_add_to_frags<PREC>), dim3((unsigned)cdiv(b.tiles * 64 * NF, 256L)), dim3(256), 0, st, b.store, VS::tile_bytes(PREC), VS::D_GEO,
                           NF, b.nsamp, b.maxbits, b.d_feature, G, G);
        EVD_LAUNCH_CHECK();
    }
    if (b.awp_store) {          // + the gradient that reached the geo features through the fused AWP embedding (awp_embed_kernel.h)
        if (G % 16) return fail(EVD_E_INVALID, "evd_voxel_mlp_backward: the AWP embedding reads the fine level (geo 128)");
        if constexpr (!is_half_prec(PREC)) return fail(EVD_E_INVALID, "evd_voxel_mlp_backward: awp_store goes with the f16 / bf16 modes (pass d_feature rows in f16x3)");
        else hipLaunchKernelGGL((k_frags_add_scaled<PREC>), dim3((unsigned)cdiv(b.tiles * 64 * (G / 16), 256L)), dim3(256), 0, st, b.store, VS::tile_bytes(PREC), VS::D_GEO,
                           b.awp_store, b.awp_tile_bytes, b.awp_slot, G / 16, b.tiles, b.maxbits, b.awp_words);
        EVD_LAUNCH_CHECK();
    }
    if ((rc = voxel_backward_inputs<PREC, VS, FT>(c, b, VOUT_DIRS))) return rc;
    // sigma_net.1 = [sigma row | geo rows] on hid
    bool sg_fused = false;
    if constexpr (FUSABLE && GT == 4) {
        // both wgrads and the dgrad in one launch -- the gradient as 4 geo row tiles + the d sigma fragment (k_wgrad_dgrad RT_ = 5, 9 k-steps): hid
        // and d geo are read once instead of three / two times (42 KiB per tile instead of 67); EVD_BWD_FUSE_SG=0: the three launches
        if (sw.fuse_sg && g.sigma_w[1]) {
            FusedExtra x;
            x.mask_slot = VS::M_HID; x.RTr = GT + 1; x.y_last_slot = VS::G_SIG;
            if ((rc = c.fused(launch_wgrad_dgrad<PREC, 8, 8, 1, GT + 1, 2 * GT + 1>, T, false, VS::D_GEO, VS::HID, VMAP_SG5, VMAP_HID, g.sigma_w[1], HD, nullptr, b.wt[VBWD_SIGGEO],
                              VS::D_HID, x))) return rc;
            sg_fused = true;
        }
    }
    if (!sg_fused) {
        if ((rc = c.wgrad(launch_wgrad<PREC, GT, T, false>, wb, GT, T, false, VS::D_GEO, VS::HID, VMAP_GEO_Y, VMAP_HID, g.sigma_w[1], HD, nullptr))) return rc;
        if ((rc = c.wgrad(launch_wgrad<PREC, 1, T, true>, wb, 1, T, false, VS::G_SIG, VS::HID, VMAP_SIG, VMAP_HID, g.sigma_w[1], HD, nullptr))) return rc;
        if ((rc = launch_dgrad<PREC, 2 * GT + 1, T, 2 * GT, true, 2>(dgrad(VBWD_SIGGEO, VS::D_GEO, VS::G_SIG, VS::M_HID, VS::D_HID), b.tiles, st))) return rc;
    }
    // sigma_net.0 on cat([fts, PE(pts)])
    bool l0_fused = false, l0_rows = false;
    if constexpr (FUSABLE && FTT == 2) {
        if (g.sigma_w[0] && (b.d_fts || b.d_pts)) {     // ... with its dgrad (d fts | d PE(pts)) in one launch
            static_assert(VS::D_PE == VS::D_FTS + 2 * FTT, "d PE(pts) behind d fts");
            l0_rows = voxel_rows_direct(b);
            FusedExtra x;
            x.rows = b.d_fts; x.rows_stride = b.d_fts_stride; x.rows_tiles = FTT;
            rc = l0_rows ? c.fused(launch_wgrad_dgrad<PREC, FTT + 2, FTT + 2, 0, 8, 16, false, true>, FTT + 2, false, VS::D_HID, VS::IN0, VMAP_HID, VMAP_FTS, g.sigma_w[0], FT + IC, nullptr,
                                   b.wt[VBWD_L0], VS::D_FTS, x)
                         : c.fused(launch_wgrad_dgrad<PREC, FTT + 2, FTT + 2, 0>, FTT + 2, false, VS::D_HID, VS::IN0, VMAP_HID, VMAP_FTS, g.sigma_w[0], FT + IC, nullptr, b.wt[VBWD_L0], VS::D_FTS);
            if (rc) return rc;
            l0_fused = true;
        }
    }
    if (l0_fused) {
    } else if constexpr (FTT == 2) {
        // the feature and encoding columns in ONE launch (their fragments and their index maps are adjacent): d hid is read once, not twice
        static_assert(VMAP_PE == VMAP_FTS + 32 * FTT, "adjacent column maps");
        if ((rc = c.wgrad(launch_wgrad<PREC, T, FTT + 2, false>, wb, T, FTT + 2, false, VS::D_HID, VS::IN0, VMAP_HID, VMAP_FTS, g.sigma_w[0], FT + IC, nullptr))) return rc;
    } else {
        if ((rc = c.wgrad(launch_wgrad<PREC, T, FTT, false>, wb, T, FTT, false, VS::D_HID, VS::IN0, VMAP_HID, VMAP_FTS, g.sigma_w[0], FT + IC, nullptr))) return rc;
        if ((rc = c.wgrad(launch_wgrad<PREC, T, 2, false>, wb, T, 2, false, VS::D_HID, VS::IN0 + KF, VMAP_HID, VMAP_PE, g.sigma_w[0], FT + IC, nullptr))) return rc;
    }
    if (b.d_fts || b.d_pts) {
        if (!l0_fused && (rc = launch_dgrad<PREC, KS, FTT + 2, KS, false, 0>(dgrad(VBWD_L0, VS::D_HID, -1, -1, VS::D_FTS), b.tiles, st))) return rc;       // d fts | d PE(pts)
        if ((rc = voxel_backward_inputs<PREC, VS, FT>(c, b, (l0_rows ? 0 : VOUT_FTS) | VOUT_PTS))) return rc;
    }
    return c.join();
}

template <int PREC, int HD, int G, int FT> static int run_voxel_backward(const VoxBwdPlan& b, hipStream_t st) {
    typedef VStore<HD, G, FT> VS;
    int rc;
    if ((rc = voxel_backward_scale(b, G, st))) return rc;
    const BwdChain c(b, VS::tile_bytes(PREC), st);
    // EVD_BWD_FUSE64=0 keeps the per-layer chain for the 64-wide level too (A/B, and the reference the fused kernel is tested against)
    if constexpr (is_half_prec(PREC) && HD == 64 && G == 15 && FT == 32) {
        if (bwd_switches().fuse64 && !b.d_feature && !b.awp_store) return voxel_backward_fused64<PREC>(c, b);
    }
    return voxel_backward_layers<PREC, HD, G, FT>(c, b);
}

}  // namespace evd
