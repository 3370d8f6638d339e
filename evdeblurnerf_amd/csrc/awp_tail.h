// AWP consumer, the PER-RAY remainder of the adaptive weight proposal: reference networks/dpnerf/awp.py:89-95 (direction
// encoding), :104-109 (motion_feature_embed_layer), networks/dpnerf/mam.py:35-53 (CorrelationModule.forward behind its per-sample part)
// and awp.py:112-115 (mean over the sub-exposures, w_linear, sigmoid, normalisation).  The reference runs ~100 launches of
// [R, 32, P]- and [R, 32, S]-sized tensors each way; here a workgroup owns a ray, keeps every intermediate of that ray in LDS
// (P <= 16 sub-exposures x 32 channels, S samples x 32 / 16 channels) and walks the whole chain:
//
//   forward   k_awp_tail_fwd     per ray: x_global, attention over P and over S, convd -> y [R,P,32]; per-workgroup sums of y, y^2 (double)
//             k_awp_tail_finish  folds the sums into the BatchNorm statistics (over ALL rays), running estimates, then per ray:
//                                normalise, residual, leaky_relu, mean over P, w_linear, sigmoid, normalise -> out [R,P]
//   backward  k_awp_tail_bwd0    per ray: d out -> d z [R,P,32]; partial sums of d gamma, d beta, d w_linear
//             k_awp_tail_bwd     per ray: BatchNorm backward with the folded sums, the forward recomputed in LDS, the chain backwards;
//                                input gradients to HBM, parameter gradients added into the workgroup's partial row
//             k_awp_tail_reduce  the partial rows -> d_params
//
// Here: sizes, a ray's LDS layout, the kernels' parameter structs, what the host entries share.  awp_tail_tile.h: device helpers;
// awp_tail_ray.h: the per-ray chains two kernels share; kernel_awp_tail.hip: forward and size queries; kernel_awp_tail_bwd.hip: backward.
#pragma once

#include "evd_common.h"

namespace evd {

constexpr int AT_WS = 64, AT_CM = 32, AT_MID = 16, AT_MAXP = 16, AT_MAXMOT = 4, AT_MAXW = 2 * AT_MAXMOT + 12;
// threads of a ray's workgroup, and how many of them share a sample row in the per-sample phases.  The working set of a ray allows one
// workgroup per CU, so the wavefronts that hide each other's LDS latency all come from here: 256 threads (one wavefront per SIMD) measured
// 66 k cycles per ray forward, 207 k backward
constexpr int AT_NT = 512, AT_LPS = 4, AT_O64 = AT_WS / AT_LPS, AT_O32 = AT_CM / AT_LPS, AT_O16 = AT_MID / AT_LPS;
constexpr int AT_LS = AT_CM + 1, AT_LK = AT_MID + 1;      // padded row strides of the per-sample LDS arrays (conflict-free row writes)
constexpr int AT_FT = 256, AT_FR = AT_FT / 32;            // threads and rays per workgroup of the finish kernels (a ray per 32 lanes)

struct TailDims {
    int P, S, VF, F, VC, IN0, n_mot, SA;                  // VC = view columns (VF + direction encoding), IN0 = 64 + VC, SA = S + 1
};

__host__ __device__ inline TailDims tail_dims(int P, int S, int VF, int F, int n_mot) {
    TailDims d;
    d.P = P; d.S = S; d.VF = VF; d.F = F; d.n_mot = n_mot;
    d.VC = VF + (F >= 0 ? 3 + 6 * F : 0);
    d.IN0 = AT_WS + d.VC;
    d.SA = S + 1;
    return d;
}

// parameter tensors in API order; sizes in floats
__host__ __device__ inline int tail_param_size(const TailDims& d, int i) {
    if (i < 2 * d.n_mot) return (i & 1) ? AT_CM : AT_CM * (i == 0 ? d.IN0 : AT_CM);
    switch (i - 2 * d.n_mot) {
        case 0: return AT_CM * AT_WS;      // MAM.linear.weight
        case 1: return AT_CM;              // MAM.linear.bias
        case 2: case 3: case 4: return AT_MID * AT_CM;      // conva, convb, convc
        case 5: case 6: return AT_MID * AT_MID;             // convn, convl
        case 7: return AT_CM * AT_CM;      // convd.0
        case 8: case 9: return AT_CM;      // convd.1 weight, bias
        case 10: return d.P * AT_CM;       // w_linear.weight
        default: return d.P;               // w_linear.bias
    }
}
enum { TW_LIN_W = 0, TW_LIN_B, TW_CONVA, TW_CONVB, TW_CONVC, TW_CONVN, TW_CONVL, TW_CONVD, TW_BN_W, TW_BN_B, TW_WL_W, TW_WL_B, TW_COUNT };

struct TailLds {
    float *mw0, *mb0, *mwr, *lin_w, *lin_b, *conva, *convb, *convc, *convn, *convl, *convd;      // mwr: layers 1.. as (W [32,32], b [32]) records
    float *x0, *xs0, *hi, *li, *kP, *nP, *q, *aP, *f, *yb;                                         // xs0: the layers' outputs, [n_mot][P][32]
    int xs_stride, ray_floats;                 // ray_floats: x0 .. aS, the ray's forward state (one contiguous block)
    __host__ __device__ float* mw(int l) const { return l == 0 ? mw0 : mwr + (l - 1) * (AT_CM * AT_CM + AT_CM); }
    __host__ __device__ float* mb(int l) const { return l == 0 ? mb0 : mwr + (l - 1) * (AT_CM * AT_CM + AT_CM) + AT_CM * AT_CM; }
    __host__ __device__ float* xs(int l) const { return xs0 + l * xs_stride; }
    float *ls, *kI, *nI, *aS;
    float *df, *daP, *dnP, *dkP, *dq, *dli, *dxa, *dxb, *daS, *dkI, *dls, *tmp;
};

// one layout for the host (size) and the device (pointers); every array starts 16-byte aligned
__host__ __device__ inline size_t tail_lds_layout(float* base, const TailDims& d, bool bwd, TailLds& L) {
    size_t at = 0;
    auto take = [&](size_t n) { float* p = base + at; at += (n + 3) & ~(size_t)3; return p; };
    L.mw0 = take((size_t)AT_CM * d.IN0); L.mb0 = take(AT_CM);
    L.mwr = take((size_t)(d.n_mot - 1) * (AT_CM * AT_CM + AT_CM));
    L.lin_w = take(AT_CM * AT_WS); L.lin_b = take(AT_CM);
    L.conva = take(AT_MID * AT_CM); L.convb = take(AT_MID * AT_CM); L.convc = take(AT_MID * AT_CM);
    L.convn = take(AT_MID * AT_MID); L.convl = take(AT_MID * AT_MID); L.convd = take(AT_CM * AT_CM);
    const size_t P = d.P;
    L.x0 = take(P * d.IN0);
    L.xs_stride = (int)(P * AT_CM);
    L.xs0 = take((size_t)d.n_mot * P * AT_CM);
    L.hi = take(P * AT_WS); L.li = take(P * AT_CM); L.kP = take(P * AT_MID); L.nP = take(P * AT_MID); L.q = take(P * AT_MID);
    L.aP = take(P * P); L.f = take(P * AT_CM); L.yb = take(P * AT_CM);
    L.ls = take((size_t)d.S * AT_LS); L.kI = take((size_t)d.S * AT_LK); L.nI = take((size_t)d.S * AT_LK); L.aS = take(P * d.SA);
    L.ray_floats = (int)(base + at - L.x0);
    L.df = L.daP = L.dnP = L.dkP = L.dq = L.dli = L.dxa = L.dxb = L.daS = L.dkI = L.dls = L.tmp = nullptr;
    if (bwd) {
        const size_t wide = d.IN0 > AT_WS ? d.IN0 : AT_WS;
        L.df = take(P * AT_CM); L.daP = take(P * P); L.dnP = take(P * AT_MID); L.dkP = take(P * AT_MID); L.dq = take(P * AT_MID);
        L.dli = take(P * AT_CM); L.dxa = take(P * wide); L.dxb = take(P * wide);
        L.daS = take(P * d.SA); L.dkI = take((size_t)d.S * AT_LK); L.dls = take((size_t)d.S * AT_LS); L.tmp = take(64);
    }
    return at;
}

// The backward kernel's static LDS, next to the ray's dynamic block; the host budgets the CU's 160 KiB with its sizeof.
struct TailBwdStatic {
    double redd[AT_NT / 64][2 * AT_CM];
    float sums[2 * AT_CM], stat[2 * AT_CM];
};
constexpr size_t AT_LDS_CU = 160 * 1024;
constexpr size_t AT_LDS_MARGIN = 512;          // spare bytes kept free next to the backward's static arrays
constexpr size_t AT_LDS_BWD_FIXED = sizeof(TailBwdStatic) + AT_LDS_MARGIN;
static_assert(AT_LDS_BWD_FIXED == 5120, "which (P, S) the entries accept is part of their contract");

struct TailKParams {
    const float* w[AT_MAXW];
    long off[AT_MAXW + 1];             // offsets of the tensors in the flat gradient buffer; [nw] = total
    TailDims d;
    int training, nw;
    float eps, momentum;
    long R;
    const float *h, *vf, *rays_d, *h_inter, *h_intra;
    float *y, *xg;                     // [R, P, 32] (forward: written; backward: read)
    float* saved;                      // [R, ray_floats]: every ray's forward state (NULL: the backward recomputes it)
    double* bn_part;                   // forward: [grid][64] sums of y, y^2
    const float *dz, *stats, *partB;   // backward
    int nblkB, partB_stride;
    long partA_stride;                 // floats between the workgroups' partial rows (a multiple of 4: the rows are 16-byte aligned)
    float *d_h, *d_vf, *d_rays, *d_hi, *d_hs, *partA;
};

struct TailFinishParams {
    const double* bn_part;
    int nparts, P, training, nblk;
    long R;
    float eps, momentum;
    const float *bn_w, *bn_b, *wl_w, *wl_b, *y, *xg;
    float *run_mean, *run_var;
    long long* num_batches;
    float *stats, *out;                // stats [64]: mean, 1 / sqrt(var + eps)
    // backward
    const float* d_out;
    float *dz, *partB;                 // partB [nblk][stride]: d beta [32], d gamma [32], d w_linear.weight [P, 32], d w_linear.bias [P]
    int partB_stride;
};

struct TailReduceParams {
    const float *partA, *partB;
    int nA, nB, partB_stride, n_tail, P;          // n_tail: elements of d_params in front of convd.1.weight
    long total, partA_stride;
    float* d_params;
};

// ---- host side: what the entries of kernel_awp_tail.hip and kernel_awp_tail_bwd.hip share ---------------------------------------------------
// the descriptor's ranges, for every entry (the size queries answer -1 / 0 where this fails)
inline bool tail_desc_ok(const evd_awp_tail_desc* d) {
    return d && d->P >= 1 && d->P <= AT_MAXP && d->S >= 1 && d->n_mot >= 1 && d->n_mot <= AT_MAXMOT && d->VF >= 0 && d->VF <= 64 && d->dir_freqs >= -1 &&
           d->dir_freqs <= 4;
}
inline TailDims tail_dims(const evd_awp_tail_desc* d) { return tail_dims(d->P, d->S, d->VF, d->dir_freqs, d->n_mot); }
inline long tail_param_total(const TailDims& dims) {
    long at = 0;
    for (int i = 0; i < 2 * dims.n_mot + TW_COUNT; ++i) at += tail_param_size(dims, i);
    return at;
}

// a launching entry's descriptor, ray count and LDS fit -> dims, the dynamic LDS bytes of its kernel
inline int tail_check(const char* who, const evd_awp_tail_desc* d, long R, bool bwd, TailDims& dims, size_t& lds_bytes) {
    EVD_REQUIRE(d, "%s: null descriptor", who);
    EVD_REQUIRE(R >= 0 && tail_desc_ok(d), "%s: P = %d (built: 1..%d), S = %d (>= 1), %d motion embedding layers (1..%d), view_feature width %d (<= 64), dir_freqs %d (-1..4)",
                who, d->P, AT_MAXP, d->S, d->n_mot, AT_MAXMOT, d->VF, d->dir_freqs);
    dims = tail_dims(d);
    TailLds L;
    lds_bytes = sizeof(float) * tail_lds_layout(nullptr, dims, bwd, L);
    const size_t fixed = bwd ? AT_LDS_BWD_FIXED : 0;
    EVD_REQUIRE(lds_bytes + fixed <= AT_LDS_CU, "%s: P = %d, S = %d needs %zu bytes of LDS per ray (the CU has 160 KiB)", who, d->P, d->S, lds_bytes + fixed);
    return EVD_OK;
}

inline int tail_grid(long R) { return (int)std::min<long>(R, device_cus()); }
inline int tail_nblk(long R) { return (int)((R + AT_FR - 1) / AT_FR); }
inline int tail_partB_stride(int P) { return 2 * AT_CM + P * AT_CM + P; }
inline long tail_partA_stride(const TailDims& dims) { return (tail_param_total(dims) + 3) & ~3L; }

// what the per-ray kernels of both directions read (y, xg, saved: written by the forward, read by the backward)
inline void tail_fill(TailKParams& k, const TailDims& dims, const evd_awp_tail_desc* d, const float* const* params, long R, const float* h, const float* view_feature,
                      const float* rays_d, const float* h_inter, const float* h_intra, const float* y, const float* xg, const float* saved_rays) {
    k.d = dims;
    k.nw = 2 * dims.n_mot + TW_COUNT;
    long at = 0;
    for (int i = 0; i < k.nw; ++i) {
        k.w[i] = params[i];
        k.off[i] = at;
        at += tail_param_size(dims, i);
    }
    k.off[k.nw] = at;
    k.training = d->training;
    k.eps = d->bn_eps;
    k.momentum = d->bn_momentum;
    k.R = R;
    k.h = h; k.vf = view_feature; k.rays_d = rays_d; k.h_inter = h_inter; k.h_intra = h_intra;
    k.y = const_cast<float*>(y); k.xg = const_cast<float*>(xg); k.saved = const_cast<float*>(saved_rays);
}
// ... and the per-ray finish of both directions (k_awp_tail_finish writes stats, k_awp_tail_bwd0 reads them)
inline void tail_fill_finish(TailFinishParams& f, const TailDims& dims, const evd_awp_tail_desc* d, const float* const* params, long R, const float* y, const float* xg,
                             const float* stats) {
    const float* const* w = params + 2 * dims.n_mot;
    f.P = dims.P; f.training = d->training; f.R = R; f.eps = d->bn_eps; f.momentum = d->bn_momentum;
    f.bn_w = w[TW_BN_W]; f.bn_b = w[TW_BN_B]; f.wl_w = w[TW_WL_W]; f.wl_b = w[TW_WL_B];
    f.y = y; f.xg = xg; f.stats = const_cast<float*>(stats);
}

// The workspaces (evd_common.h Workspace: one layout for the size query and for the carve) and the grids that size them
struct TailFwdWs { int grid; double* bn_part; };                       // [grid][64] sums of y, y^2
struct TailBwdWs { int grid, nblk; float *dz, *partB, *partA; };       // d z [R, P, 32] | k_awp_tail_bwd0's rows | k_awp_tail_bwd's rows
constexpr size_t TAIL_FWD_WS_SLACK = 256, TAIL_BWD_WS_SLACK = 256;      // alignment slack for an unaligned caller pointer
inline size_t tail_fwd_layout(long R, void* workspace, TailFwdWs* L) {
    Workspace ws(workspace);
    L->grid = tail_grid(R > 0 ? R : 1);
    L->bn_part = ws.take<double>(2 * AT_CM * (size_t)L->grid);
    return ws.used() + TAIL_FWD_WS_SLACK;
}
inline size_t tail_bwd_layout(const TailDims& dims, long R, void* workspace, TailBwdWs* L) {
    Workspace ws(workspace);
    L->grid = tail_grid(R > 0 ? R : 1); L->nblk = tail_nblk(R);
    L->dz = ws.take<float>((size_t)R * dims.P * AT_CM);
    L->partB = ws.take<float>((size_t)L->nblk * tail_partB_stride(dims.P));
    L->partA = ws.take<float>((size_t)L->grid * (size_t)tail_partA_stride(dims));
    return ws.used() + TAIL_BWD_WS_SLACK;
}

}  // namespace evd
