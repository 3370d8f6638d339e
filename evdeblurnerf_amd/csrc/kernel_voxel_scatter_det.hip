// The tri-plane scatter in its DETERMINISTIC form (evd_voxel_sample_bwd_det; answers the reference's seed_everything(..., deterministic=True),
// run_nerf.py:50, where its own grid_sample backward, voxnerf.py:144, cannot).  The float atomics of kernel_voxel_sample_bwd.hip and
// kernel_voxel_scatter.hip make the last bits of the plane / line gradients depend on the order in which the hardware retires them.  Here
// every tap contribution w_tap x (d coef x other) is computed in float32 as there, converted to 64-bit FIXED POINT with ONE power-of-two
// unit for the whole call and added to a shadow accumulator with an integer atomic: integer addition is associative, the sum does not
// depend on the order.  A finish kernel converts each accumulator once and adds it to the caller's gradient.
//   pass 0  k_voxel_scatter_det<0>: the same contributions, not added; their largest magnitude by atomicMax on the float's bits
//           (a maximum is associative too).  The host takes the unit from it: evd_scatter_det_unit_exp.
//   pass 1  k_voxel_scatter_det<1>: the adds, the point gradient (a fixed shuffle tree over the channels of a sample) and the basis_mat
//           gradient (register partials per workgroup, tile t always on workgroup t mod gridDim, written to the workspace)
//   finish  k_scatter_det_finish (shadow -> gradients, accumulators left zero), k_scatter_det_basis (workgroup partials in workgroup order)
// A sample's contributions are a function of that sample alone (d coef is a float32 fmaf chain over app_dim, no per-tile scale), so the plane
// and line gradients are invariant under any permutation of the samples; the basis_mat gradient is reproducible for a given n only.
// Layout as the block-cooperative form: 32-sample tiles, lanes over channels, so a wavefront's atomics cover contiguous runs of one tap.
#include "voxel_taps.h"

namespace evd {

constexpr int SD_TAPS = 18;             // per sample: 3 x 4 plane + 3 x 2 line
constexpr int SD_MAXF = 64;
constexpr int SD_BATCH = 4;             // samples whose taps are in flight together in the gather phase (divides 16)
constexpr int SD_BLOCKS = 512;          // workgroups of the scatter passes at most: a constant, so that the tile -> workgroup map depends on n only
constexpr size_t SD_LDS_MAX = 96 * 1024;

struct DetShadow { unsigned long long *plane[3], *line[3]; };       // null = that gradient is not wanted

template <int PASS, bool HALF>
__global__ __launch_bounds__(256) void k_voxel_scatter_det(const GridParams g, const float* __restrict__ pts, long n,
                                                           const float* __restrict__ d_out, int d_stride, int d_col, DetShadow sh,
                                                           float* __restrict__ d_pts, float* __restrict__ bpart, unsigned* __restrict__ cmax, float up) {
    extern __shared__ __attribute__((aligned(16))) float sd_smem[];
    __shared__ float tw[VS_SAMPLES * SD_TAPS], tfr[VS_SAMPLES * 3 * 6], dpart[VS_SAMPLES * 2 * 3];
    __shared__ long tix[VS_SAMPLES * SD_TAPS];
    __shared__ int tvm[VS_SAMPLES * 3];
    const int c0n = g.n_comp[0], c1n = g.n_comp[1], ctot = c0n + c1n + g.n_comp[2], F = g.app_dim, nbas = F * ctot;
    const int ST = ctot | 1, FS = F | 1;              // odd row strides
    float* bas = sd_smem;                             // basis_mat [F][ctot]
    float* dout = bas + nbas;                         // [32][FS]
    float* dco = dout + VS_SAMPLES * FS;              // d coef [32][ST]
    float* pvs = dco + VS_SAMPLES * ST;               // plane value, line value [32][ST]
    float* lvs = pvs + VS_SAMPLES * ST;
    const int tid = threadIdx.x, ss = tid >> 7, ql = tid & 127, lane = tid & 63, half_w = (tid >> 6) & 1;
    // this thread's channel in the gather sweeps: component, channel inside it
    const int cg = ql < c0n ? 0 : (ql < c0n + c1n ? 1 : 2), cin = ql - (cg == 0 ? 0 : (cg == 1 ? c0n : c0n + c1n));
    const bool chan_on = ql < ctot;
    const float* gplane = sel3(cg, g.plane[0], g.plane[1], g.plane[2]);
    const float* gline = sel3(cg, g.line[0], g.line[1], g.line[2]);
    const _Float16* hplane = sel3(cg, g.plane_h[0], g.plane_h[1], g.plane_h[2]);
    const _Float16* hline = sel3(cg, g.line_h[0], g.line_h[1], g.line_h[2]);
    // ... and its (tap, channel) entries in the scatter sweeps: q = ql + 128 m over [4 plane taps x ctot | 2 line taps x ctot]
    constexpr int MQ = (6 * VS_MAXC + 127) / 128;
    int q_slot[MQ], q_c[MQ];
    unsigned long long* q_ptr[MQ];
    bool q_plane[MQ];
#pragma unroll
    for (int m = 0; m < MQ; ++m) {
        const int q = ql + 128 * m;
        const bool on = q < 6 * ctot, pl = q < 4 * ctot;
        const int t = pl ? q / ctot : (q - 4 * ctot) / ctot, c = q % ctot;
        const ChannelOf ch = channel_component(c, c0n, c1n);
        q_plane[m] = pl;
        q_c[m] = c;
        q_slot[m] = pl ? 4 * ch.i + t : 12 + 2 * ch.i + t;
        unsigned long long* base = pl ? sel3(ch.i, sh.plane[0], sh.plane[1], sh.plane[2]) : sel3(ch.i, sh.line[0], sh.line[1], sh.line[2]);
        q_ptr[m] = (on && base) ? base + ch.c : nullptr;
    }
    // the basis_mat gradient of this workgroup's tiles: thread (ss, ql) owns channel ql and the features ss, ss + 2, ...
    constexpr int NB = SD_MAXF / 2;
    float bacc[NB];
#pragma unroll
    for (int q = 0; q < NB; ++q) bacc[q] = 0.f;
    float mx = 0.f;                                   // pass 0: the largest |contribution| this lane saw (NaN recorded as +inf)
    for (int o = tid; o < nbas; o += 256) bas[o] = g.basis[o];          // (made visible by the first tile's barrier)
    for (long tile = blockIdx.x; tile * VS_SAMPLES < n; tile += gridDim.x) {
        const long s0 = tile * VS_SAMPLES;
        for (int o = tid; o < VS_SAMPLES * F; o += 256) {
            const int sl = o / F, f = o % F;
            dout[sl * FS + f] = s0 + sl < n ? d_out[(s0 + sl) * (long)d_stride + d_col + f] : 0.f;
        }
        if (tid < VS_SAMPLES * 3) {                   // tap table: thread = (sample, component)
            const int sl = tid / 3, i = tid % 3;
            const bool live = s0 + sl < n;
            const long s = live ? s0 + sl : n - 1;
            const float pt[3] = {pts[s * 3], pts[s * 3 + 1], pts[s * 3 + 2]};
            const TapGeom tg = tap_geometry(g, pt, i);
            Taps<long> tp;                            // ip / il address channel 0 of the tap
            tap_offsets_weights<long>(tg, live, tp);
            const TapGrad e = tap_grad(g, tg, i, live);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                tix[sl * SD_TAPS + 4 * i + t] = tp.ip[t];
                tw[sl * SD_TAPS + 4 * i + t] = tp.wp[t];
            }
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                tix[sl * SD_TAPS + 12 + 2 * i + t] = tp.il[t];
                tw[sl * SD_TAPS + 12 + 2 * i + t] = tp.wl[t];
            }
            float* fr = tfr + (sl * 3 + i) * 6;
            fr[0] = e.fw; fr[1] = e.fn; fr[2] = e.fl; fr[3] = e.kx; fr[4] = e.ky; fr[5] = e.kl;
            tvm[sl * 3 + i] = e.vm;
        }
        __syncthreads();
        // d coef[s, c] = sum_f d out[s, f] basis[f, c]: one float32 fmaf chain per element, a function of the sample's row alone
        for (int o = tid; o < VS_SAMPLES * ctot; o += 256) {
            const int sl = o / ctot, c = o % ctot;
            float a = 0.f;
            for (int f = 0; f < F; ++f) a = fmaf(dout[sl * FS + f], bas[f * ctot + c], a);
            dco[sl * ST + c] = a;
        }
        __syncthreads();
        // pv, lv: lanes over channels, two samples per sweep (a sample's channels lie on two wavefronts: half_w); the taps of SD_BATCH
        // samples are loaded before the first is used (one sample at a time the tile is a chain of 16 load latencies)
        for (int b0 = 0; b0 < VS_SAMPLES / 2; b0 += SD_BATCH) {
        float Pb[SD_BATCH][4], Lb[SD_BATCH][2];
        if (chan_on) {
#pragma unroll
            for (int j = 0; j < SD_BATCH; ++j) {
                const long* ti = tix + (ss + 2 * (b0 + j)) * SD_TAPS;
#pragma unroll
                for (int t = 0; t < 4; ++t) Pb[j][t] = HALF ? (float)hplane[ti[4 * cg + t] + cin] : gplane[ti[4 * cg + t] + cin];
#pragma unroll
                for (int t = 0; t < 2; ++t) Lb[j][t] = HALF ? (float)hline[ti[12 + 2 * cg + t] + cin] : gline[ti[12 + 2 * cg + t] + cin];
            }
        }
#pragma unroll
        for (int j = 0; j < SD_BATCH; ++j) {
            const int sl = ss + 2 * (b0 + j);
            float vx = 0.f, vy = 0.f, vz = 0.f;
            if (chan_on) {
                const float* w = tw + sl * SD_TAPS;
                float P[4], Lt[2], pv = 0.f, lv = 0.f;
#pragma unroll
                for (int t = 0; t < 4; ++t) P[t] = Pb[j][t];
#pragma unroll
                for (int t = 0; t < 2; ++t) Lt[t] = Lb[j][t];
#pragma unroll
                for (int t = 0; t < 4; ++t) pv = fmaf(w[4 * cg + t], P[t], pv);
#pragma unroll
                for (int t = 0; t < 2; ++t) lv = fmaf(w[12 + 2 * cg + t], Lt[t], lv);
                pvs[sl * ST + ql] = pv;
                lvs[sl * ST + ql] = lv;
                if (PASS == 1 && d_pts) {
                    // d feature / d point through the interpolation weights (the ATen grid_sample backward: a tap outside the grid is a
                    // zero VALUE, decided by the validity mask, not by the weight), chained with d coef
                    const float* fr = tfr + (sl * 3 + cg) * 6;
                    const float ww = fr[0], nn = fr[1], ee = 1.f - ww, sn = 1.f - nn;
                    const int vm = tvm[sl * 3 + cg];
#pragma unroll
                    for (int t = 0; t < 4; ++t) P[t] = (vm >> t) & 1 ? P[t] : 0.f;
                    const float dpx = (P[1] - P[0]) * sn + (P[3] - P[2]) * nn, dpy = (P[2] - P[0]) * ee + (P[3] - P[1]) * ww;
                    const float dl = ((vm >> 5) & 1 ? Lt[1] : 0.f) - ((vm >> 4) & 1 ? Lt[0] : 0.f);
                    const float dc = dco[sl * ST + ql];
                    const float gx = dc * lv * dpx * fr[3], gy = dc * lv * dpy * fr[4], gl = dc * pv * dl * fr[5];
                    // component i feeds the axes (ax, ay | al) = (0, 1 | 2), (0, 2 | 1), (1, 2 | 0)
                    vx = cg == 2 ? gl : gx;
                    vy = cg == 0 ? gy : (cg == 1 ? gl : gx);
                    vz = cg == 0 ? gl : gy;
                }
            }
            if (PASS == 1 && d_pts) {
                // the sum over the sample's channels in a FIXED order: a butterfly over the wavefront's 64 lanes (lanes without a channel
                // hold 0), then the two wavefronts of the sample in order (below).  No LDS atomics.
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) { vx += __shfl_xor(vx, o); vy += __shfl_xor(vy, o); vz += __shfl_xor(vz, o); }
                if (lane == 0) {
                    float* dp = dpart + (sl * 2 + half_w) * 3;
                    dp[0] = vx; dp[1] = vy; dp[2] = vz;
                }
            }
        }
        }
        __syncthreads();
        // the taps: contribution = d coef x other x w in float32, as the direct forms compute it.  (Tried and dropped: a thread walking 16
        // consecutive samples with the integer sum of a run of samples on one cell in registers, one atomic per run -- the same sums, fewer
        // requests, and pass 1 of a training iteration's nine scatters went from 21.2 to 42.5 ms: the walk is a chain of dependent LDS
        // reads and compares, as kernel_voxel_sample_bwd.hip found for the float form.)
        for (int sl = ss; sl < VS_SAMPLES; sl += 2) {
#pragma unroll
            for (int m = 0; m < MQ; ++m) {
                if (!q_ptr[m]) continue;
                const float w = tw[sl * SD_TAPS + q_slot[m]];
                if (w == 0.f) continue;
                const int c = q_c[m];
                const float other = q_plane[m] ? lvs[sl * ST + c] : pvs[sl * ST + c];
                const float v = dco[sl * ST + c] * other * w;
                if (PASS == 0) {
                    const float a = fabsf(v);
                    mx = a != a ? __builtin_huge_valf() : fmaxf(mx, a);
                } else {
                    const long long fx = __float2ll_rn(v * up);
                    if (fx != 0) atomicAdd(q_ptr[m] + tix[sl * SD_TAPS + q_slot[m]], (unsigned long long)fx);
                }
            }
        }
        if (PASS == 1) {
            if (d_pts && tid < VS_SAMPLES * 3 && s0 + tid / 3 < n) {
                const int sl = tid / 3, a = tid % 3;
                d_pts[(s0 + sl) * 3 + a] = dpart[(sl * 2) * 3 + a] + dpart[(sl * 2 + 1) * 3 + a];
            }
            if (bpart && chan_on) {                   // d basis[f, c] += sum_s d out[s, f] pv lv, in registers across this workgroup's tiles
#pragma unroll 1
                for (int sl = 0; sl < VS_SAMPLES; ++sl) {
                    const float cf = pvs[sl * ST + ql] * lvs[sl * ST + ql];
                    const float* dr = dout + sl * FS + ss;
#pragma unroll
                    for (int q = 0; q < NB; ++q)
                        if (ss + 2 * q < F) bacc[q] = fmaf(dr[2 * q], cf, bacc[q]);
                }
            }
        }
        __syncthreads();
    }
    if (PASS == 0) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        const unsigned mb = __float_as_uint(mx);      // (non-negative floats order like their bit patterns; +inf above all)
        if (lane == 0 && mb != 0u) atomicMax(cmax, mb);
    } else if (bpart && chan_on) {
#pragma unroll
        for (int q = 0; q < NB; ++q)
            if (ss + 2 * q < F) bpart[(long)blockIdx.x * nbas + (ss + 2 * q) * ctot + ql] = bacc[q];
    }
}

// shadow -> gradient: grad[i] += (float)(acc[i] 2^-k), one conversion and one float32 add per element; the accumulator is left zero
struct DetSeg { unsigned long long* acc; float* grad; long n; };
struct DetSegs { DetSeg s[6]; };
static __global__ __launch_bounds__(256) void k_scatter_det_finish(const DetSegs segs, double down) {
    const DetSeg s = segs.s[blockIdx.y];
    if (!s.acc) return;
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < s.n; i += stride) {
        const long long a = (long long)s.acc[i];
        if (a != 0) {
            s.grad[i] += (float)((double)a * down);
            s.acc[i] = 0ull;
        }
    }
}

// the workgroups' basis_mat partials, folded in workgroup order (the k_wgrad_reduce pattern)
static __global__ __launch_bounds__(256) void k_scatter_det_basis(const float* __restrict__ bpart, int blocks, int nbas, float* __restrict__ grad) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= nbas) return;
    float a = 0.f;
    int b = 0;
    for (; b + 8 <= blocks; b += 8) {                 // eight loads in flight, added in workgroup order
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = bpart[(long)(b + j) * nbas + o];
#pragma unroll
        for (int j = 0; j < 8; ++j) a += v[j];
    }
    for (; b < blocks; ++b) a += bpart[(long)b * nbas + o];
    grad[o] += a;
}

static const int kDM0[3] = {0, 0, 1}, kDM1[3] = {1, 2, 2}, kDV[3] = {2, 1, 0};
// [max word, 256 B] [shadow: the six accumulator arrays, each 256-byte aligned] [basis partials: SD_BLOCKS x app_dim x ctot floats]
struct DetRegion { unsigned* cmax; unsigned long long* acc[6]; long elems[6]; float* bpart; };     // (aligned by the caller, who adds the slack for that)
static size_t det_region_layout(const GridParams& g, void* region, DetRegion* L) {
    Workspace ws(region);
    L->cmax = ws.take<unsigned>(1);
    for (int i = 0; i < 3; ++i) { L->elems[i] = (long)g.grid[kDM0[i]] * g.grid[kDM1[i]] * g.n_comp[i]; L->elems[3 + i] = (long)g.grid[kDV[i]] * g.n_comp[i]; }
    for (int k = 0; k < 6; ++k) L->acc[k] = ws.take<unsigned long long>((size_t)L->elems[k]);
    L->bpart = ws.take<float>((size_t)SD_BLOCKS * g.app_dim * (g.n_comp[0] + g.n_comp[1] + g.n_comp[2]));
    return ws.used();
}
size_t voxel_scatter_det_region_bytes(const GridParams& g) { DetRegion L; return det_region_layout(g, nullptr, &L); }

struct DetPlan {
    DetShadow sh;
    DetSegs segs;
    unsigned* cmax;
    float* bpart;
    size_t zero_bytes;          // the max word + the shadow: what pass 0 clears, from cmax on
    unsigned blocks;
    size_t lds;
};

static int det_plan(const GridParams& g, long n, const GridGrads& gg, void* region, DetPlan& p) {
    if (g.app_dim > SD_MAXF) return fail(EVD_E_INVALID, "evd_voxel_sample_bwd_det: app_dim %d > %d", g.app_dim, SD_MAXF);
    const int ctot = g.n_comp[0] + g.n_comp[1] + g.n_comp[2];
    if (ctot > VS_MAXC) return fail(EVD_E_INVALID, "evd_voxel_sample_bwd_det: sum(n_comp) %d > %d", ctot, VS_MAXC);
    DetRegion L;
    det_region_layout(g, region, &L);
    p.cmax = L.cmax; p.bpart = gg.basis ? L.bpart : nullptr; p.zero_bytes = (size_t)((char*)L.bpart - (char*)L.cmax);
    for (int k = 0; k < 6; ++k) {
        float* grad = k < 3 ? gg.plane[k] : gg.line[k - 3];
        unsigned long long* acc = grad ? L.acc[k] : nullptr;
        (k < 3 ? p.sh.plane[k] : p.sh.line[k - 3]) = acc;
        p.segs.s[k] = DetSeg{acc, grad, L.elems[k]};
    }
    const long tiles = cdiv(n, (long)VS_SAMPLES);
    p.blocks = (unsigned)(tiles < SD_BLOCKS ? tiles : SD_BLOCKS);
    p.lds = ((size_t)g.app_dim * ctot + (size_t)VS_SAMPLES * (g.app_dim | 1) + (size_t)3 * VS_SAMPLES * (ctot | 1)) * sizeof(float);
    if (p.lds > SD_LDS_MAX) return fail(EVD_E_INVALID, "evd_voxel_sample_bwd_det: %zu bytes of LDS > %zu", p.lds, SD_LDS_MAX);
    return EVD_OK;
}

#define EVD_SD(PASS, H, ...) { EVD_SET_MAX_LDS((&k_voxel_scatter_det<PASS, H>), SD_LDS_MAX); \
        k_voxel_scatter_det<PASS, H><<<p.blocks, 256, p.lds, st>>>(__VA_ARGS__); }

// pass 0: zero shadow and maximum word, then the largest |contribution| of the batch -> the word at the start of the region
int launch_voxel_scatter_det_scale(const GridParams& g, bool half_grids, const float* pts, long n, const float* d_out, int d_stride, int d_col,
                                   const GridGrads& gg, void* region, hipStream_t st) {
    DetPlan p;
    int rc = det_plan(g, n, gg, region, p);
    if (rc) return rc;
    EVD_HIP(hipMemsetAsync(p.cmax, 0, p.zero_bytes, st));
    if (half_grids) EVD_SD(0, true, g, pts, n, d_out, d_stride, d_col, p.sh, nullptr, nullptr, p.cmax, 0.f)
    else EVD_SD(0, false, g, pts, n, d_out, d_stride, d_col, p.sh, nullptr, nullptr, p.cmax, 0.f)
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

// pass 1 + the finish kernels with the unit 2^-k
int launch_voxel_scatter_det_add(const GridParams& g, bool half_grids, const float* pts, long n, const float* d_out, int d_stride, int d_col,
                                 const GridGrads& gg, float* d_pts, void* region, int k, hipStream_t st) {
    DetPlan p;
    int rc = det_plan(g, n, gg, region, p);
    if (rc) return rc;
    const float up = ldexpf(1.f, k);
    if (half_grids) EVD_SD(1, true, g, pts, n, d_out, d_stride, d_col, p.sh, d_pts, p.bpart, p.cmax, up)
    else EVD_SD(1, false, g, pts, n, d_out, d_stride, d_col, p.sh, d_pts, p.bpart, p.cmax, up)
    EVD_LAUNCH_CHECK();
    long nmax = 0;
    bool any = false;
    for (int i = 0; i < 6; ++i)
        if (p.segs.s[i].acc) { any = true; nmax = p.segs.s[i].n > nmax ? p.segs.s[i].n : nmax; }
    if (any) {
        const long bx = cdiv(nmax, 256L) < 2048 ? cdiv(nmax, 256L) : 2048;
        hipLaunchKernelGGL(k_scatter_det_finish, dim3((unsigned)bx, 6), dim3(256), 0, st, p.segs, ldexp(1.0, -k));
        EVD_LAUNCH_CHECK();
    }
    if (gg.basis) {
        const int nbas = g.app_dim * (g.n_comp[0] + g.n_comp[1] + g.n_comp[2]);
        hipLaunchKernelGGL(k_scatter_det_basis, dim3((unsigned)cdiv(nbas, 256L)), dim3(256), 0, st, p.bpart, (int)p.blocks, nbas, gg.basis);
        EVD_LAUNCH_CHECK();
    }
    return EVD_OK;
}
#undef EVD_SD

}  // namespace evd
