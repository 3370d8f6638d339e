// PDRF backbone: the backward of the tri-plane feature gather (kernel_voxel_sample.hip) -- the scatter into the plane, line and basis_mat
// gradients and the point gradient -- in its block-cooperative and its wavefront-autonomous form.  The line taps of the hybrid scatter and
// its driver are in kernel_voxel_scatter.hip.
#include "voxel_taps.h"
#include "wave_ops.h"

namespace evd {

// Backward of k_voxel_sample (app_act none): d out [n, app_dim] -> gradients of the planes, lines (scatter-add, the transpose of
// the gather: the same 4 + 2 taps with the same weights) and of basis_mat.  Persistent blocks walk 32-sample tiles; inside a
// tile the LANES RUN OVER CHANNELS (the grids are channel-last), so every gather and every atomic of a wavefront covers
// contiguous 64..256-byte runs of one tap:
//   A  d out rows -> LDS;  d coef[s, c] = sum_f d out[s, f] basis[f, c];  tap table (18 per sample: 3 x 4 plane + 3 x 2 line)
//   B  plane value pv[s, c], line value lv[s, c] (coalesced gathers), then
//      d plane[tap, c] += w_tap d coef lv,  d line[tap, c] += w_tap d coef pv  as hardware float32 atomics (global_atomic_add_f32);
//      like the reference's grid_sample backward (voxnerf.py:144) the summation order, hence the last bits, is not deterministic
//   C  d basis[f, c] += sum_s d out[s, f] pv lv in registers across tiles, one atomic flush per block at the end
// Measured (fine level, 2^19 samples, 302 M float atomics): **1.23 ms = 246 G adds/s**, the hardware rate of one dword per clock per L2
// channel (128 channels).  Round 1: 1.45 ms (1.80 ms with the two small GEMMs on the VALU).  Round 2: the kernel compiled to 256 VGPRs
// + 109 AGPRs under a loose launch bound, i.e. ONE block per CU, and its non-atomic work (0.98 ms: per-tile latency chain of point
// load, tap table, GEMM, gathers) barely hid under the atomics; with the VALU fallback's accumulators templated out (MM) and
// __launch_bounds__(256, 2) it takes 172 VGPRs, two blocks per CU share the latency, and the gather sweep is unrolled 4 x:
// 1.43 -> 1.23 ms, whole blurfactory iteration 32.6 -> 28.9 ms.  Plane-only and line-only variants
// cost the same per add, and 32 private copies of the (heavily shared) line gradients change nothing: it is the op count, not
// contention.  Tried and dropped: a run-length sum over the tile's consecutive samples that hit the same cell before the atomic (one
// thread per (tap, channel) walking the 32 samples): the sequential walk costs more than the adds it saves (3.1 ms) unless the rays
// run along a grid axis.  Also tried and dropped (round 2): per-tile LDS windows (8 x 8 plane cells / 32 line cells around the tile's
// taps, ds_add_f32, one global atomic per touched cell) for the components whose taps stay together along a ray -- the bounding-box
// atomics, the per-tap window index and the flush add ~0.5 ms per 2^19 samples to this one-wavefront-per-SIMD kernel and the whole
// blurfactory iteration went from 33.2 to 42.1 ms; and the sort + LDS-tile form of kernel_voxel_scatter.hip (2 x slower as built).
// And, once ds_add_f32 was known to be the slow part (kernel_voxel_scatter.hip), the same window for the 64-channel x-y plane WITHOUT
// atomics (lane = channel, a window cell owned by one wavefront, every wavefront walks the tile's 128 (sample, tap) entries in order;
// the box of the benchmark's NDC rays is 42-60 cells, 22-28 of them touched by the 128 taps): correct, and 0.92 -> 1.43 ms per 2^19
// samples, iteration 22.6 -> 30.3 ms -- the walk is a chain of dependent LDS read-modify-writes, again.
constexpr int VSB_MAXF = 64, VSB_TAPS = 18;
constexpr int VSB_BATCH = 4;            // samples whose taps are in flight together in the gather phase of k_voxel_sample_bwd (divides 16)
// CT: the channel capacity the LDS rows are laid out for (MM: ctot <= CT, a multiple of 32).  With the shipped 96 channels and
// app_dim 32 the block needs 50 KB of LDS and 168 VGPRs = three blocks per CU.  (Measured: three blocks run at the speed of two,
// 1.21 ms = 249 G adds/s; a bare kernel of coalesced float atomics on random 64-byte runs sustains 318 - 328 G adds/s = 20 G requests/s
// regardless of the table size, tools/probes/atomic_probe.hip, and the counters show EVERY atomic request of this kernel travelling to
// the memory side, TCC_EA0_ATOMIC == TCC_ATOMIC = 18.6 M 64-byte requests per 2^19 samples: device-scope float atomics are not
// executed in the XCD's L2.  The kernel is at 78 % of that ceiling; the gap is the repeated hits on the same few line cells.)

// HYBRID = false: every tap by a direct atomic.  HYBRID = true: the plane taps by direct atomics, the line taps deferred -- their rows
// (rows_l) and tap records (ltap) are written and k_scatter_lines adds them through privatised LDS slices of the (small) line gradients:
// a third of the kernel's atomic requests go away.
template <bool HYBRID, bool MM, int CT>
__global__ __launch_bounds__(256, MM ? (CT <= 96 ? 3 : 2) : 1) void k_voxel_sample_bwd(const GridParams g, const float* __restrict__ pts, long n,
                                                          const float* __restrict__ d_out, int d_stride, int d_col, GridGrads gg,
                                                          float* __restrict__ d_pts, float* rows_l, LTap* ltap) {
    constexpr int STRD = CT + 1, FSTR = MM ? 33 : VSB_MAXF + 1;      // odd row strides (conflict-free column access)

    __shared__ float tfr[VS_SAMPLES * 3 * 6], dpt[VS_SAMPLES * 3];
    __shared__ int tax[VS_SAMPLES * 3 * 4];           // axes of the component's three coordinates + the tap validity mask
    __shared__ __attribute__((aligned(16))) float pvs[VS_SAMPLES * STRD], lvs[VS_SAMPLES * STRD], dco[VS_SAMPLES * STRD],
        dout[VS_SAMPLES * FSTR], tw[VS_SAMPLES * VSB_TAPS];
    __shared__ int tix[VS_SAMPLES * VSB_TAPS];
    const int c0n = g.n_comp[0], c1n = g.n_comp[1], ctot = c0n + c1n + g.n_comp[2], F = g.app_dim, nbas = F * ctot;
    const int tid = threadIdx.x, ss = tid >> 7, ql = tid & 127;
    // this thread's channel in the (sample pair, 128 channel slots) sweeps of phase B: component group, channel inside it
    const int cg = ql < c0n ? 0 : (ql < c0n + c1n ? 1 : 2), cin = ql - (cg == 0 ? 0 : (cg == 1 ? c0n : c0n + c1n));
    const bool chan_on = ql < ctot;
    const bool rows16 = (c0n % 16 == 0) && (c1n % 16 == 0) && (g.n_comp[2] % 16 == 0);     // components = whole 16-lane DPP rows
    const float* gplane = sel3(cg, g.plane[0], g.plane[1], g.plane[2]);
    const float* gline = sel3(cg, g.line[0], g.line[1], g.line[2]);
    // ... and its (tap, channel) entries in the atomic sweeps: q = ql + 128 m over [4 plane taps x ctot | 2 line taps x ctot]
    constexpr int MQ = (6 * VS_MAXC + 127) / 128;
    int q_slot[MQ], q_c[MQ];
    float* q_ptr[MQ];
    bool q_plane[MQ];
#pragma unroll
    for (int m = 0; m < MQ; ++m) {
        const int q = ql + 128 * m;
        const bool on = q < 6 * ctot, pl = q < 4 * ctot;
        const int t = pl ? q / ctot : (q - 4 * ctot) / ctot, c = q % ctot;
        const int i = c < c0n ? 0 : (c < c0n + c1n ? 1 : 2), ci = c - (i == 0 ? 0 : (i == 1 ? c0n : c0n + c1n));
        q_plane[m] = pl;
        q_c[m] = c;
        q_slot[m] = pl ? 4 * i + t : 12 + 2 * i + t;
        float* base = pl ? sel3(i, gg.plane[0], gg.plane[1], gg.plane[2]) : sel3(i, gg.line[0], gg.line[1], gg.line[2]);
        q_ptr[m] = (on && base) ? base + ci : nullptr;
    }
    constexpr int NB = (VSB_MAXF * VS_MAXC + 255) / 256;
    float bacc[NB];
#pragma unroll
    for (int q = 0; q < NB; ++q) bacc[q] = 0.f;
    // The two small GEMMs of a tile (d coef = d out . basis and d basis += d out^T . coef: 32 x 32 x ctot each) run on the exact-float32
    // MFMA when app_dim is 32 and the channels come in 32-wide tiles: wavefront t owns channel tile t for both (on the VALU the second
    // one costs three LDS reads per multiply-add: 19 GB of LDS traffic per 2^19 samples).
    const int wv = tid >> 6, ln = tid & 63, mn = ln & 31, kb = ln >> 5;
    // MM (template: keeps the VALU fallback's 32 accumulators out of the common instantiation, which then fits two blocks per CU)
    const bool mm = MM, mm_wave = mm && wv * 32 < ctot;
    float bas_reg[16];
    f32x16 macc;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        macc[r] = 0.f;
        bas_reg[r] = mm_wave ? g.basis[(long)(2 * r + kb) * ctot + 32 * wv + mn] : 0.f;
    }
    for (long tile = blockIdx.x; tile * VS_SAMPLES < n; tile += gridDim.x) {
        const long s0 = tile * VS_SAMPLES;
        for (int o = tid; o < VS_SAMPLES * F; o += 256) {
            const int sl = o / F, f = o % F;
            dout[sl * FSTR + f] = s0 + sl < n ? d_out[(s0 + sl) * (long)d_stride + d_col + f] : 0.f;
        }
        if (tid < VS_SAMPLES * 3) {                // tap table: thread = (sample, component group)
            const int sl = tid / 3, i = tid % 3;
            const long s = s0 + sl < n ? s0 + sl : n - 1;
            const float pt[3] = {pts[s * 3], pts[s * 3 + 1], pts[s * 3 + 2]};
            const bool live = s0 + sl < n;
            // OPTIMISATION BARRIER, not arithmetic: ic == i (every n_comp is a positive multiple of 4; for other widths ic is what the
            // channel decode of the component's first group gives, as this step has always computed it).  With tap_geometry(g, pt, i)
            // hipcc proves the component's selections and kx / ky / kl invariant, carries them through the tile loop in ~20 more
            // registers, and the two 96-channel instances spill 32 / 30 VGPRs at their 168-register bound; through the decode they
            // spill 2 / 0 (this file before the tap geometry was shared: 4 / 2).  An empty asm with a "+v" constraint on i was tried
            // in its place: 8 / 2.  Do not replace it by i without reading the spill counts of <*, true, 96>.
            const int grp0 = i == 0 ? 0 : (i == 1 ? c0n / 4 : (c0n + c1n) / 4);
            const int ic = channel_component(grp0 * 4, c0n, c1n).i;
            const TapGeom tg = tap_geometry(g, pt, ic);
            Taps<int> tp;                           // ip / il address channel 0 of the tap
            tap_offsets_weights<long>(tg, live, tp);          // <long> into an int record: offsets computed in 64 bits, then truncated, as this kernel always has
            const TapGrad e = tap_grad(g, tg, ic, live);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                tix[sl * VSB_TAPS + 4 * i + t] = tp.ip[t];
                tw[sl * VSB_TAPS + 4 * i + t] = tp.wp[t];
            }
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                tix[sl * VSB_TAPS + 12 + 2 * i + t] = tp.il[t];
                tw[sl * VSB_TAPS + 12 + 2 * i + t] = tp.wl[t];
            }
            float* fr = tfr + (sl * 3 + i) * 6;
            fr[0] = e.fw; fr[1] = e.fn; fr[2] = e.fl; fr[3] = e.kx; fr[4] = e.ky; fr[5] = e.kl;
            int* ta = tax + (sl * 3 + i) * 4;
            ta[0] = e.ax; ta[1] = e.ay; ta[2] = e.al; ta[3] = e.vm;
            if constexpr (HYBRID) {
                if (live) {                         // the line taps of this (sample, component), for k_scatter_lines
                    const int C = tg.C;
                    LTap lt_;
                    lt_.c0 = tp.il[0] / C; lt_.c1 = tp.il[1] / C; lt_.w0 = tp.wl[0]; lt_.w1 = tp.wl[1];
                    ltap[s * 3 + i] = lt_;
                }
            }
        }
        if (tid < VS_SAMPLES * 3) dpt[tid] = 0.f;
        __syncthreads();
        if (mm) {
            if (mm_wave) {                          // D[sample][channel] = sum_f d out[sample][f] basis[f][channel]
                f32x16 a16;
#pragma unroll
                for (int r = 0; r < 16; ++r) a16[r] = 0.f;
#pragma unroll
                for (int j = 0; j < 16; ++j) a16 = __builtin_amdgcn_mfma_f32_32x32x2f32(dout[mn * FSTR + 2 * j + kb], bas_reg[j], a16, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 16; ++r) dco[((r & 3) + 8 * (r >> 2) + 4 * kb) * STRD + 32 * wv + mn] = a16[r];
            }
        } else {
            for (int o = tid; o < VS_SAMPLES * ctot; o += 256) {
                const int sl = o / ctot, c = o % ctot;
                float a = 0.f;
                for (int f = 0; f < F; ++f) a = fmaf(dout[sl * FSTR + f], g.basis[(long)f * ctot + c], a);
                dco[sl * STRD + c] = a;
            }
        }
        if (d_pts) __syncthreads();                 // the point gradient below reads d coef
        if (chan_on) {                              // pv, lv: lanes over channels, two samples per sweep
            // The taps of VSB_BATCH samples are loaded before the first is used.  (As one loop with "#pragma unroll 4" hipcc left it rolled --
            // the DPP row sums and LDS atomics of the d pts part are convergent operations --: six loads, then a wait for all six, 16 times
            // per tile, and in-kernel stamps put half of a tile's time in this phase.)
            for (int b0 = 0; b0 < VS_SAMPLES / 2; b0 += VSB_BATCH) {
            float Pb[VSB_BATCH][4], Lb[VSB_BATCH][2];
#pragma unroll
            for (int j = 0; j < VSB_BATCH; ++j) {
                const int* ti = tix + (ss + 2 * (b0 + j)) * VSB_TAPS;
#pragma unroll
                for (int t = 0; t < 4; ++t) Pb[j][t] = gplane[ti[4 * cg + t] + cin];
#pragma unroll
                for (int t = 0; t < 2; ++t) Lb[j][t] = gline[ti[12 + 2 * cg + t] + cin];
            }
#pragma unroll
            for (int j = 0; j < VSB_BATCH; ++j) {
                const int sl = ss + 2 * (b0 + j);
                const int* ti = tix + sl * VSB_TAPS;
                const float* w = tw + sl * VSB_TAPS;
                float pv = 0.f, lv = 0.f, P[4], Lt[2];
#pragma unroll
                for (int t = 0; t < 4; ++t) { P[t] = Pb[j][t]; pv = fmaf(w[4 * cg + t], P[t], pv); }
#pragma unroll
                for (int t = 0; t < 2; ++t) { Lt[t] = Lb[j][t]; lv = fmaf(w[12 + 2 * cg + t], Lt[t], lv); }
                pvs[sl * STRD + ql] = pv;
                lvs[sl * STRD + ql] = lv;
                if (d_pts) {
                    // d feature / d point through the interpolation weights (the ATen grid_sample backward: a tap outside the grid is a zero
                    // VALUE -- decided by the validity mask, not by the weight: at an exact integer index the upper tap is inside with weight 0
                    // and its value enters the derivative), chained with d coef; summed over the channels of the wavefront, then over
                    // wavefronts in LDS
                    const float* fr = tfr + (sl * 3 + cg) * 6;
                    const float ww = fr[0], nn = fr[1], ee = 1.f - ww, sn = 1.f - nn;
                    const int vm = tax[(sl * 3 + cg) * 4 + 3];
#pragma unroll
                    for (int t = 0; t < 4; ++t) P[t] = (vm >> t) & 1 ? P[t] : 0.f;
                    const float dpx = (P[1] - P[0]) * sn + (P[3] - P[2]) * nn, dpy = (P[2] - P[0]) * ee + (P[3] - P[1]) * ww;
                    const float dl = ((vm >> 5) & 1 ? Lt[1] : 0.f) - ((vm >> 4) & 1 ? Lt[0] : 0.f);
                    const float dc = dco[sl * STRD + ql];
                    float gx = dc * lv * dpx * fr[3], gy = dc * lv * dpy * fr[4], gl = dc * pv * dl * fr[5];
                    // sum over the component's channels.  When every component is a whole number of 16-lane rows (the shipped 64 / 16 / 16)
                    // the rows are summed in registers (DPP) and ONE lane per row adds to LDS: 18 LDS float atomics per sample instead of
                    // 288 -- ds_add_f32 runs at ~0.4 lane-operations per clock and CU on this chip (kernel_voxel_scatter.hip), so the
                    // 9216 of a tile cost more than everything else the tile does
                    const int* ta = tax + (sl * 3 + cg) * 4;
                    if (rows16) {
                        gx = row_sum_dpp(gx); gy = row_sum_dpp(gy); gl = row_sum_dpp(gl);
                        if ((tid & 15) == 0) {
                            atomicAdd(&dpt[sl * 3 + ta[0]], gx);
                            atomicAdd(&dpt[sl * 3 + ta[1]], gy);
                            atomicAdd(&dpt[sl * 3 + ta[2]], gl);
                        }
                    } else {
                        atomicAdd(&dpt[sl * 3 + ta[0]], gx);
                        atomicAdd(&dpt[sl * 3 + ta[1]], gy);
                        atomicAdd(&dpt[sl * 3 + ta[2]], gl);
                    }
                }
            }
            }
        }
        __syncthreads();
        // (Re-measured in round 2 with the half-tile walk that keeps a ray's runs together -- successive samples of an NDC ray address
        // ~12 distinct x-y cells and ~7 x / y line cells per 32 samples --: summing the run in a register before ONE atomic is 1.5-1.9x
        // SLOWER, 2.76 vs 1.46 ms at 2^19 samples: the walk is a chain of dependent LDS reads, the sweep below is not.)
        if constexpr (HYBRID) {
            if (chan_on) {
                for (int sl = ss; sl < VS_SAMPLES && s0 + sl < n; sl += 2) rows_l[(s0 + sl) * ctot + ql] = dco[sl * STRD + ql] * pvs[sl * STRD + ql];
            }
        }
        for (int sl = ss; sl < VS_SAMPLES; sl += 2) {
#pragma unroll
            for (int m = 0; m < MQ; ++m) {
                if (!q_ptr[m] || (HYBRID && !q_plane[m])) continue;
                const float w = tw[sl * VSB_TAPS + q_slot[m]];
                if (w == 0.f) continue;
                const int c = q_c[m];
                const float other = q_plane[m] ? lvs[sl * STRD + c] : pvs[sl * STRD + c];
                unsafeAtomicAdd(q_ptr[m] + tix[sl * VSB_TAPS + q_slot[m]], dco[sl * STRD + c] * other * w);
            }
        }
        if (d_pts && tid < VS_SAMPLES * 3 && s0 + tid / 3 < n) d_pts[(s0 + tid / 3) * 3 + tid % 3] = dpt[tid];
        if (gg.basis && mm) {
            if (mm_wave) {                          // D[f][channel] += sum_s d out[s][f] coef[s][channel]
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int sl = 2 * j + kb;
                    macc = __builtin_amdgcn_mfma_f32_32x32x2f32(dout[sl * FSTR + mn],
                                                                pvs[sl * STRD + 32 * wv + mn] * lvs[sl * STRD + 32 * wv + mn], macc, 0, 0, 0);
                }
            }
        } else if (gg.basis) {
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                const int o = tid + 256 * q;
                if (o < nbas) {
                    const int f = o / ctot, c = o % ctot;
                    float a = bacc[q];
                    for (int sl = 0; sl < VS_SAMPLES; ++sl) a = fmaf(dout[sl * FSTR + f], pvs[sl * STRD + c] * lvs[sl * STRD + c], a);
                    bacc[q] = a;
                }
            }
        }
        __syncthreads();
    }
    if (gg.basis && mm) {
        if (mm_wave) {
#pragma unroll
            for (int r = 0; r < 16; ++r) unsafeAtomicAdd(gg.basis + (long)((r & 3) + 8 * (r >> 2) + 4 * kb) * ctot + 32 * wv + mn, macc[r]);
        }
    } else if (gg.basis) {
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            const int o = tid + 256 * q;
            if (o < nbas) unsafeAtomicAdd(gg.basis + o, bacc[q]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// k_voxel_sample_bwd_w: the backward gather WAVEFRONT-AUTONOMOUS, like the forward's k_voxel_sample_w.  In-kernel stamps of the block-cooperative
// kernel above put half of a tile's time in its gather phase and showed the whole kernel to be a per-tile latency chain (point load, tap
// table, GEMM, gathers, four block barriers) that stays at ~0.72 ms per 2^19 samples even with two thirds of its atomics removed.  Here a
// WAVEFRONT owns 16 consecutive samples (of one ray, as the renderer lays them out) from the point load to its last atomic; the one
// block barrier orders the basis_mat image in LDS:
//   0  tap geometry of its 48 (sample, component) pairs on 48 lanes -> its LDS slice (+ the line tap records for k_scatter_lines)
//   1  d coef^T = basis^T . d out^T on v_mfma_f32_16x16x32_f16 in the split-float16 form (3 MFMAs per 16-channel tile; d out as the
//      register-resident B operand)
//   2  the gather exactly as the forward does it: 3 items (sample, 8 channels) per lane, 36 16-byte loads in flight, then per item
//      pv, lv;  line rows d coef pv -> HBM (k_scatter_lines);  coef = pv lv -> LDS;  plane rows d coef lv -> LDS in place;
//      the point gradient's per-item partial sums -> LDS
//   3  the plane taps, lanes over channels (every atomic instruction covers whole 64-byte runs).  A 64-channel component (the x-y
//      plane) is walked sample by sample with the sum kept in a REGISTER while successive samples address the same cell -- the rays of an
//      NDC scene run along z, a tile's 16 samples touch 1-4 x-y cells -- and flushed by one atomic per (run, tap); the 16 / 32-channel
//      components (their taps move with every sample) add tap by tap
//   4  the point gradient: 48 lanes sum the partials of their (sample, axis)
//   5  the basis_mat gradient d out^T . coef of the tile's samples, accumulated in registers across the wavefront's tiles
// The line taps go through k_scatter_lines as in the block-cooperative hybrid form.
constexpr int VBW_SAMPLES = 16, VBW_WAVES = 4;
constexpr int VBW_BSTR = 112;                   // basis_mat row stride in LDS: 16 (mod 32) words, so that the MFMA A reads (lane = channel + 16 x row step) hit 64 banks
constexpr int VBW_CSTR = 97;                    // d coef / plane-row stride (ctot <= 96), odd: lanes over channels read conflict-free
constexpr int VBW_MAXG = 12;                    // 8-channel groups per sample
struct VbwTaps {
    int ip[4], il[2];                           // element offsets of channel 0 of the taps (clamped)
    float wp[4], wl[2];                         // interpolation weights, 0 = outside (zero padding) or dead sample
    float fw, fn, kx, ky, kl;                   // fractional position in the plane cell; d (pixel coordinate) / d (point coordinate)
    int vm;                                     // taps inside the grid (TapGrad::vm; 0 for a dead sample): the point gradient's zero padding
};
// a wavefront's slice: tap tables | d coef -> plane rows [16][CSTR] | point-gradient partial sums [16][3 quads][3] | the coefficient rows
// pv lv [16][96] of the in-kernel basis gradient.  16 KiB per wavefront: two workgroups of four per CU (2 x 78 KiB of the 160 KiB)
constexpr int VBW_FSTR = 96;                    // coefficient row stride: the MFMA B reads (32 channels x 2 samples per step) cover the 64 banks
constexpr size_t VBW_SLICE = VBW_SAMPLES * 3 * sizeof(VbwTaps) + (size_t)VBW_SAMPLES * VBW_CSTR * 4 + (size_t)VBW_SAMPLES * 9 * 4 + (size_t)VBW_SAMPLES * VBW_FSTR * 4;
static_assert(VBW_MAXG * 8 <= VBW_FSTR, "a sample's coefficients fit its row");
constexpr size_t VBW_LDS = (size_t)32 * VBW_BSTR * 4 + VBW_WAVES * VBW_SLICE;
static_assert(sizeof(VbwTaps) % 8 == 0 && VBW_SLICE % 16 == 0, "slice alignment");

// The basis_mat gradient d out^T . coef INSIDE this kernel.  The workgroups are persistent (a wavefront walks tiles
// blockIdx.x, blockIdx.x + gridDim.x, ...: basis_mat is staged in LDS once per workgroup instead of once per 64 samples), a wavefront leaves
// the coefficients pv lv of its gather items in its slice (cfl) and adds its 16 samples' [F x ctot] product to 3 x 16 accumulator registers on
// v_mfma_f32_32x32x2_f32 (d out rows as the A operand straight from L2); one fold through LDS + one atomic flush per workgroup at the end.
// (Coefficient rows [n, ctot] in HBM for a separate GEMM kernel would be 201 MB written and read back per 2^19 samples, and a launch.)
// The plane-tap walk (phase 3 of k_voxel_sample_bwd_w): a lane owns a (tap, channel), walks the tile's 16 samples with the sum of a RUN of
// samples on one cell in a register and adds it once per run.  The kernel is bound by the number of instructions its two wavefronts per
// SIMD issue (~5.5 k per tile and wavefront, 4 cycles each; a build WITHOUT the atomics showed the walk alone at 33.6 k of a tile's 51.8 k
// cycles, profiles/r06_scatter_stamps_before_walk_rewrite.log: the "atomic phase" was this loop, not the atomics), so the walk is cut to what
// it needs:
//   * all LDS operands of a pass are fetched first (independent reads), the walk runs on registers;
//   * weight x row with the legacy multiply (0 x anything = 0): the same sums as the guarded form `w != 0 ? w * r : 0` -- a tap
//     outside the grid (weight 0) adds nothing even where the row is not finite -- without a compare and a select per step;
//   * a run whose sum is exactly 0 in a lane adds nothing (x + 0 = x): no separate `any sample live` flag is kept.
// vbw_walk_pass: one tap per lane group (a 16-channel plane: all four taps in one pass of 64 lanes).
template <class FW, class FC, class FR>
__device__ __forceinline__ void vbw_walk_pass(float* __restrict__ gp, int c, bool act, FW fw, FC fc, FR fr) {
    float w[VBW_SAMPLES], r[VBW_SAMPLES];
    int cell[VBW_SAMPLES];
#pragma unroll
    for (int sm = 0; sm < VBW_SAMPLES; ++sm) { w[sm] = fw(sm); cell[sm] = fc(sm); r[sm] = fr(sm); }
    float acc = 0.f;
#pragma unroll
    for (int sm = 0; sm < VBW_SAMPLES; ++sm) {
        acc += mul_legacy(w[sm], r[sm]);
        const bool flush = sm == VBW_SAMPLES - 1 || cell[sm + 1 < VBW_SAMPLES ? sm + 1 : sm] != cell[sm];
        if (flush) {
            if (act && acc != 0.f) unsafeAtomicAdd(gp + cell[sm] + c, acc);
            acc = 0.f;
        }
    }
}

// vbw_walk_plane64: the 64-channel plane, lane = channel, ALL FOUR taps in one pass.  The taps of a sample are the corners of one cell, so
// the four cell indices change together: the run ends are the steps where tap 0's or tap 3's index changes (both unchanged <=> the
// clamped corner pairs (x0, y0) and (x1, y1) unchanged <=> all four unchanged), decided on two scalar registers per sample.  Per step: four
// multiplies and four adds; the row value is read once instead of four times.
template <class FW4, class FC, class FR>
__device__ __forceinline__ void vbw_walk_plane64(float* __restrict__ gp, int c, FW4 fw4, FC fc, FR fr) {
    float r[VBW_SAMPLES];
    f32x4 w[VBW_SAMPLES];
    int c0[VBW_SAMPLES], c3[VBW_SAMPLES];
#pragma unroll
    for (int sm = 0; sm < VBW_SAMPLES; ++sm) { w[sm] = fw4(sm); c0[sm] = fc(sm, 0); c3[sm] = fc(sm, 3); r[sm] = fr(sm); }
#pragma unroll
    for (int sm = 0; sm < VBW_SAMPLES; ++sm) { c0[sm] = __builtin_amdgcn_readfirstlane(c0[sm]); c3[sm] = __builtin_amdgcn_readfirstlane(c3[sm]); }
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int sm = 0; sm < VBW_SAMPLES; ++sm) {
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] += mul_legacy(w[sm][t], r[sm]);
        const int nx = sm + 1 < VBW_SAMPLES ? sm + 1 : sm;
        const bool flush = sm == VBW_SAMPLES - 1 || c0[nx] != c0[sm] || c3[nx] != c3[sm];
        if (flush) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int cell = fc(sm, t);
                if (acc[t] != 0.f) unsafeAtomicAdd(gp + cell + c, acc[t]);
                acc[t] = 0.f;
            }
        }
    }
}

// HALF: phase 2 re-gathers the grid values from the FLOAT16 copies (GridParams::plane_h / line_h) -- the values the forward of the
// half-precision arithmetic modes interpolated (voxel_net.h grids_half_for), so the products d coef x value are the gradient of the function
// that forward computed; half the gather's loads and bytes, weight x value + sum as one v_fma_mix_f32 on the float16 value (as k_voxel_sample_m).
template <bool DPTS, bool HALF>
__global__ __launch_bounds__(64 * VBW_WAVES, 2) void k_voxel_sample_bwd_w(const GridParams g, const float* __restrict__ pts, long n,
                                                                          const float* __restrict__ d_out, int d_stride, int d_col, GridGrads gg,
                                                                          float* __restrict__ d_pts, float* __restrict__ rows_l, LTap* __restrict__ ltap,
                                                                          unsigned* __restrict__ lmax) {
    extern __shared__ __attribute__((aligned(16))) char vbw_smem[];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c0n = g.n_comp[0], c1n = g.n_comp[1], c2n = g.n_comp[2], ctot = c0n + c1n + c2n, F = g.app_dim;
    float* bs = reinterpret_cast<float*>(vbw_smem);                                  // basis_mat [32][VBW_BSTR], rows >= F are zero
    char* slice = vbw_smem + (size_t)32 * VBW_BSTR * 4 + (size_t)wv * VBW_SLICE;
    VbwTaps* taps = reinterpret_cast<VbwTaps*>(slice);
    float* dco = reinterpret_cast<float*>(slice + VBW_SAMPLES * 3 * sizeof(VbwTaps));   // d coef [16][VBW_CSTR], later the plane rows d coef lv
    float* dpart = dco + VBW_SAMPLES * VBW_CSTR;                                     // [16][3 quads of 8-channel groups][3 axes] d pts partial sums
    float* cfl = dpart + VBW_SAMPLES * 9;                                            // [16][VBW_FSTR] coefficients pv lv
    const int ng = ctot / 8;
    // basis_mat -> LDS (the block's only shared state) as the A operands of phase 1: d coef^T = basis^T . d out^T on
    // v_mfma_f32_16x16x32_f16 in the split form (hi = f16(x), lo = f16(x - hi): A_hi B_hi + A_hi B_lo + A_lo B_hi, 2^-21 per product) --
    // 18 MFMAs of 16 cycles per tile instead of 48 float32 16 x 16 x 4 of 32.  Entry (channel tile ct, lane): basis[8 (lane / 16) + j][16 ct + lane % 16],
    // j = 0 .. 7; the region is the one the block's fold of the basis gradient uses at the end (bs).  float16 has 5 exponent bits and gradients
    // are small, so both operands are brought to [2^13, 2^14) by a power of two first -- one per channel (row of A, kept in a1_inv) and
    // one per sample (column of B, pow2_scale_f16 on the row's largest magnitude) -- and the product is scaled back exactly.
    f16x8* a1_hi = reinterpret_cast<f16x8*>(bs);                                     // [6][64]
    f16x8* a1_lo = a1_hi + 6 * 64;
    float* a1_inv = reinterpret_cast<float*>(a1_lo + 6 * 64);                        // [96]
    static_assert((size_t)2 * 6 * 64 * 16 + 96 * 4 <= (size_t)32 * VBW_BSTR * 4, "the split operands fit the fold buffer");
    for (int e = threadIdx.x; e < 6 * 64; e += 64 * VBW_WAVES) {                     // whole wavefronts: the shuffles below see all four k groups of a channel
        const int l = e & 63, ct = e >> 6, ch = 16 * ct + (l & 15), f0 = 8 * (l >> 4);
        float v[8], m = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            v[j] = (f0 + j < F && ch < ctot) ? g.basis[(long)(f0 + j) * ctot + ch] : 0.f;
            m = fmaxf(m, fabsf(v[j]));
        }
        m = fmaxf(m, __shfl_xor(m, 16));
        m = fmaxf(m, __shfl_xor(m, 32));
        float inv;
        const float sc = pow2_scale_f16(m, &inv);
        f16x8 hi, lo;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float x = v[j] * sc;
            hi[j] = (_Float16)x;
            lo[j] = (_Float16)(x - (float)hi[j]);
        }
        a1_hi[e] = hi;
        a1_lo[e] = lo;
        if (l < 16) a1_inv[ch] = inv;
    }
    __syncthreads();                              // the only block-wide barrier in front of the tiles: basis_mat visible
    auto wave_sync = []() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); };
    constexpr int NCT = 3;                        // 32-channel tiles of the basis gradient (ctot <= 96)
    f32x16 bacc[NCT];
#pragma unroll
    for (int c = 0; c < NCT; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) bacc[c][r] = 0.f;
    float rmaxv = 0.f;                            // max |line row value| this lane wrote (k_scatter_lines' fixed-point scale: saves it a pass over the rows)
    const long wtiles = (n + VBW_SAMPLES - 1) / VBW_SAMPLES;
    for (long wt = (long)blockIdx.x * VBW_WAVES + wv; wt < wtiles; wt += (long)gridDim.x * VBW_WAVES) {
    const long s0 = wt * VBW_SAMPLES;
    // d out as the MFMA B operand: lane (col = sample, kh) holds d out[sample][4 step + kh]
    const int col = lane & 15, kh = lane >> 4;
    float dv[8];                                  // lane (col = sample, kh): d out[sample][8 kh .. 8 kh + 7]
    {
        const long s = s0 + col;
        const float* r = d_out + (s < n ? s : n - 1) * (long)d_stride + d_col;
#pragma unroll
        for (int j = 0; j < 8; ++j) dv[j] = (s < n && 8 * kh + j < F) ? r[8 * kh + j] : 0.f;
    }
    if (lane < VBW_SAMPLES * 3) {                 // phase 0: geometry of this wavefront's (sample, component) pairs
        const int sl = lane / 3, i = lane % 3;
        const bool live = s0 + sl < n;
        const long s = live ? s0 + sl : n - 1;
        const float pt[3] = {pts[s * 3], pts[s * 3 + 1], pts[s * 3 + 2]};
        const TapGeom tg = tap_geometry(g, pt, i);
        const TapGrad e = tap_grad(g, tg, i, live);
        VbwTaps tp;
        tap_offsets_weights<int>(tg, live, tp);
        tp.fw = e.fw; tp.fn = e.fn; tp.kx = e.kx; tp.ky = e.ky; tp.kl = e.kl; tp.vm = e.vm;
        taps[lane] = tp;
        if (live && ltap) {
            const int C = sel3(i, c0n, c1n, c2n);
            LTap lt_;
            lt_.c0 = tp.il[0] / C; lt_.c1 = tp.il[1] / C; lt_.w0 = tp.wl[0]; lt_.w1 = tp.wl[1];
            ltap[s * 3 + i] = lt_;
        }
    }
    wave_sync();                                  // the tap tables are the wavefront's own
    // phase 1: D[channel 16 ct + 4 kh + r][sample col] = sum_f basis[f][channel] d out[sample][f]
    {
        float m = 0.f, binv;
#pragma unroll
        for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf(dv[j]));
        m = fmaxf(m, __shfl_xor(m, 16));
        m = fmaxf(m, __shfl_xor(m, 32));
        const float bsc = pow2_scale_f16(m, &binv);
        f16x8 bh, bl;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float x = dv[j] * bsc;
            bh[j] = (_Float16)x;
            bl[j] = (_Float16)(x - (float)bh[j]);
        }
        for (int ct = 0; ct < ctot / 16; ++ct) {
            const f16x8 ah = a1_hi[ct * 64 + lane], al = a1_lo[ct * 64 + lane];
            const f32x4 ai = *reinterpret_cast<const f32x4*>(a1_inv + 16 * ct + 4 * kh);
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, acc, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = acc[r] * ai[r] * binv;
#pragma unroll
            for (int r = 0; r < 4; ++r) dco[col * VBW_CSTR + 16 * ct + 4 * kh + r] = acc[r];
        }
    }
    wave_sync();
    // phase 2: gather, 3 items per lane in flight
    const int items = VBW_SAMPLES * ng;
    // items in flight per lane and trip: three (144 registers of raw taps) -- two where the wavefront also carries the basis accumulators
    // (48 registers) AND the point gradient's operands: at three that form spills 27 registers into the tile loop
    constexpr int UNR = (DPTS && !HALF) ? 2 : 3, TRIPS = 3 / UNR + (3 % UNR ? 1 : 0);      // (HALF: 24 instead of 48 registers of raw taps per item)
#pragma unroll
    for (int trip = 0; trip < TRIPS; ++trip) {
        const int base = lane + trip * UNR * 64;
        if (base >= items) break;
        f32x4 rawp[UNR][4][2], rawl[UNR][2][2];
        f16x8 hfp[UNR][4], hfl[UNR][2];           // HALF: the taps' eight float16 values (one 16-byte load each)
        int sl[UNR], grp[UNR], comp[UNR];
        bool on[UNR];
#pragma unroll
        for (int q = 0; q < UNR; ++q) {
            const int t = base + q * 64;
            on[q] = t < items;
            sl[q] = on[q] ? t / ng : 0;
            grp[q] = on[q] ? t % ng : 0;
            const ChannelOf ch = channel_component(grp[q] * 8, c0n, c1n);
            const int i = ch.i, c8 = ch.c;
            comp[q] = i;
            const VbwTaps& tp = taps[sl[q] * 3 + i];
            if (HALF) {
                const _Float16* plh = sel3(i, g.plane_h[0], g.plane_h[1], g.plane_h[2]) + c8;
                const _Float16* lih = sel3(i, g.line_h[0], g.line_h[1], g.line_h[2]) + c8;
#pragma unroll
                for (int k = 0; k < 4; ++k) hfp[q][k] = *reinterpret_cast<const f16x8*>(plh + tp.ip[k]);
#pragma unroll
                for (int k = 0; k < 2; ++k) hfl[q][k] = *reinterpret_cast<const f16x8*>(lih + tp.il[k]);
            } else {
                const float* pl = sel3(i, g.plane[0], g.plane[1], g.plane[2]) + c8;
                const float* li = sel3(i, g.line[0], g.line[1], g.line[2]) + c8;
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int v = 0; v < 2; ++v) rawp[q][k][v] = *reinterpret_cast<const f32x4*>(pl + tp.ip[k] + 4 * v);
#pragma unroll
                for (int k = 0; k < 2; ++k)
#pragma unroll
                    for (int v = 0; v < 2; ++v) rawl[q][k][v] = *reinterpret_cast<const f32x4*>(li + tp.il[k] + 4 * v);
            }
        }
#pragma unroll
        for (int q = 0; q < UNR; ++q) {
            const VbwTaps& tp = taps[sl[q] * 3 + comp[q]];
            const bool live = on[q] && s0 + sl[q] < n;
            const int cb = grp[q] * 8;
            float* drow = dco + sl[q] * VBW_CSTR + cb;
            float gx = 0.f, gy = 0.f, gl = 0.f;
            const float ww = tp.fw, nn = tp.fn, ee = 1.f - ww, sn = 1.f - nn;
#pragma unroll
            for (int v = 0; v < 2; ++v) {
                f32x4 pv = {0.f, 0.f, 0.f, 0.f}, lv = {0.f, 0.f, 0.f, 0.f};
                // (w != 0 ? pv + raw w : pv as pv + legacy(w, raw) -- the same value, a tap outside the grid (w = 0) adds 0 whatever
                // lies at its clamped address -- one instruction less per element in a kernel bound by the instructions it issues)
                auto plane_val = [&](int t, int k) __attribute__((always_inline)) { return HALF ? (float)hfp[q][t][4 * v + k] : rawp[q][t][v][k]; };
                auto line_val = [&](int t, int k) __attribute__((always_inline)) { return HALF ? (float)hfl[q][t][4 * v + k] : rawl[q][t][v][k]; };
                if (HALF && DPTS) {               // the converted values are needed for the point gradient anyway: conversions + packed FMAs
#pragma unroll
                    for (int t = 0; t < 4; ++t)
#pragma unroll
                        for (int k = 0; k < 4; ++k) pv[k] = __builtin_fmaf(tp.wp[t], plane_val(t, k), pv[k]);
#pragma unroll
                    for (int t = 0; t < 2; ++t)
#pragma unroll
                        for (int k = 0; k < 4; ++k) lv[k] = __builtin_fmaf(tp.wl[t], line_val(t, k), lv[k]);
                } else if (HALF) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const u32x4 pw = __builtin_bit_cast(u32x4, hfp[q][t]);
#pragma unroll
                        for (int k = 0; k < 4; k += 2) {
                            pv[k] = fma_mix_f16<0>(tp.wp[t], pw[2 * v + (k >> 1)], pv[k]);
                            pv[k + 1] = fma_mix_f16<1>(tp.wp[t], pw[2 * v + (k >> 1)], pv[k + 1]);
                        }
                    }
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        const u32x4 lw = __builtin_bit_cast(u32x4, hfl[q][t]);
#pragma unroll
                        for (int k = 0; k < 4; k += 2) {
                            lv[k] = fma_mix_f16<0>(tp.wl[t], lw[2 * v + (k >> 1)], lv[k]);
                            lv[k + 1] = fma_mix_f16<1>(tp.wl[t], lw[2 * v + (k >> 1)], lv[k + 1]);
                        }
                    }
                } else {
#pragma unroll
                    for (int t = 0; t < 4; ++t)
#pragma unroll
                        for (int k = 0; k < 4; ++k) pv[k] = __fadd_rn(pv[k], mul_legacy(tp.wp[t], plane_val(t, k)));
#pragma unroll
                    for (int t = 0; t < 2; ++t)
#pragma unroll
                        for (int k = 0; k < 4; ++k) lv[k] = __fadd_rn(lv[k], mul_legacy(tp.wl[t], line_val(t, k)));
                }
                f32x4 dc, rl, cf, rp;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    dc[k] = drow[4 * v + k];
                    rl[k] = dc[k] * pv[k];
                    cf[k] = pv[k] * lv[k];
                    rp[k] = dc[k] * lv[k];
                }
                if (live && rows_l) {
                    *reinterpret_cast<f32x4*>(rows_l + (s0 + sl[q]) * ctot + cb + 4 * v) = rl;
                    if (lmax) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const float a = fabsf(rl[k]);
                            rmaxv = a != a ? __builtin_huge_valf() : fmaxf(rmaxv, a);       // (a NaN is recorded as +inf)
                        }
                    }
                }
                if (on[q]) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) cfl[sl[q] * VBW_FSTR + cb + 4 * v + k] = cf[k];
#pragma unroll
                    for (int k = 0; k < 4; ++k) drow[4 * v + k] = rp[k];
                }
                if (DPTS) {
                    // d feature / d point through the interpolation weights (the ATen grid_sample backward: a tap outside the grid is a zero
                    // VALUE; inside-ness from the mask, not the weight -- at an exact integer index the upper tap is inside with weight 0),
                    // chained with d coef
                    const int vm = tp.vm;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float P0 = vm & 1 ? plane_val(0, k) : 0.f, P1 = vm & 2 ? plane_val(1, k) : 0.f;
                        const float P2 = vm & 4 ? plane_val(2, k) : 0.f, P3 = vm & 8 ? plane_val(3, k) : 0.f;
                        const float dpx = (P1 - P0) * sn + (P3 - P2) * nn, dpy = (P2 - P0) * ee + (P3 - P1) * ww;
                        const float dl = (vm & 32 ? line_val(1, k) : 0.f) - (vm & 16 ? line_val(0, k) : 0.f);
                        gx += dc[k] * lv[k] * dpx;
                        gy += dc[k] * lv[k] * dpy;
                        gl += dc[k] * pv[k] * dl;
                    }
                }
            }
            if (DPTS) {
                // component i feeds the axes (ax, ay | al) = (0, 1 | 2), (0, 2 | 1), (1, 2 | 0): into axis space, then summed over the quad
                // (four consecutive 8-channel groups of one sample: ng = 12 groups are three whole quads, items and lanes are quad-aligned)
                // in registers -- a quarter of the partial sums go through LDS
                const int i = comp[q];
                const float a0 = on[q] ? gx * tp.kx : 0.f, a1 = on[q] ? gy * tp.ky : 0.f, a2 = on[q] ? gl * tp.kl : 0.f;
                float vx = i == 2 ? a2 : a0, vy = i == 0 ? a1 : (i == 1 ? a2 : a0), vz = i == 0 ? a2 : a1;
                vx += dpp_f32<0xb1>(0.f, vx); vy += dpp_f32<0xb1>(0.f, vy); vz += dpp_f32<0xb1>(0.f, vz);
                vx += dpp_f32<0x4e>(0.f, vx); vy += dpp_f32<0x4e>(0.f, vy); vz += dpp_f32<0x4e>(0.f, vz);
                if (on[q] && (lane & 3) == 0) {
                    float* dp = dpart + (sl[q] * 3 + (grp[q] >> 2)) * 3;
                    dp[0] = vx; dp[1] = vy; dp[2] = vz;
                }
            }
        }
    }
    wave_sync();
    // the A operand of the basis gradient's MFMAs (d out[sample 2 u + kb][f = lane & 31]) is fetched HERE, in front of the plane taps'
    // atomics: the VM counter retires in order, a load issued behind them waits for every one of them (stamps: the 24 MFMAs of phase 5 took
    // 14 k cycles with their eight loads issued one by one behind the atomics, a fifth of the tile)
    float bav[VBW_SAMPLES / 2];
    {
        const int mn = lane & 31, kb = lane >> 5;
#pragma unroll
        for (int u = 0; u < VBW_SAMPLES / 2; ++u) {
            const long sa = s0 + 2 * u + kb;
            bav[u] = (sa < n && mn < F) ? d_out[sa * (long)d_stride + d_col + mn] : 0.f;
        }
        // ... and waited for here (an L2 hit: the rows were read for phase 1): hipcc cannot count the atomics of the loops below, at the
        // MFMAs it would wait for vmcnt(0).  (Also tried: the NEXT tile's d out / point loads issued here as well -- 0.556 ms either way:
        // the kernel runs at the rate its atomics retire, a wait moved is not a wait removed.)
#pragma unroll
        for (int u = 0; u < VBW_SAMPLES / 2; ++u) asm volatile("" : "+v"(bav[u]));
    }
    // phase 3: plane taps.  dco now holds the plane rows d coef lv.
    int coff = 0;
#pragma unroll 1
    for (int i = 0; i < 3; ++i) {
        const int C = sel3(i, c0n, c1n, c2n);
        float* gp = sel3(i, gg.plane[0], gg.plane[1], gg.plane[2]);
        if (gp) {
            // lanes = (tap, channel): 64 / C taps of the component per pass (one for the 64-channel x-y plane, all four for a 16-channel
            // plane).  Every lane walks the tile's 16 samples with the sum of a RUN of samples on one cell in a register and adds it once
            // per run: the x-y cell of an NDC ray changes every ~10 samples, and where the importance samples cluster at a surface the
            // x-z / y-z cells repeat as well
            const int tpp = 64 / C < 4 ? 64 / C : 4, j = lane / C, c = lane % C;
            if (C == 64) {
                vbw_walk_plane64(gp, lane, [&](int sm) { const f32x2 a = *reinterpret_cast<const f32x2*>(taps[sm * 3 + i].wp), b = *reinterpret_cast<const f32x2*>(taps[sm * 3 + i].wp + 2);
                                                         return f32x4{a[0], a[1], b[0], b[1]}; },
                                 [&](int sm, int t) { return taps[sm * 3 + i].ip[t]; }, [&](int sm) { return dco[sm * VBW_CSTR + coff + lane]; });
            } else {
#pragma unroll 1
                for (int t0 = 0; t0 < 4; t0 += tpp) {
                    const int t = t0 + (j < tpp ? j : 0);
                    vbw_walk_pass(gp, c, j < tpp, [&](int sm) { return taps[sm * 3 + i].wp[t]; }, [&](int sm) { return taps[sm * 3 + i].ip[t]; },
                                  [&](int sm) { return dco[sm * VBW_CSTR + coff + c]; });
                }
            }
        }
        coff += C;
    }
    // phase 4: the point gradient of (sample, axis): the three quads' partial sums
    if (DPTS && lane < VBW_SAMPLES * 3) {
        const int sl = lane / 3, a = lane % 3;
        float sum = 0.f;
        for (int qd = 0; qd < (ng + 3) / 4; ++qd) sum += dpart[(sl * 3 + qd) * 3 + a];
        if (s0 + sl < n) d_pts[(s0 + sl) * 3 + a] = sum;
    }
    {
        // phase 5: d basis_mat += d out^T . coef over the tile's 16 samples (coefficient rows: written to the slice by phase 2)
        const int mn = lane & 31, kb = lane >> 5;
#pragma unroll
        for (int u = 0; u < VBW_SAMPLES / 2; ++u) {
            const float av = bav[u];
#pragma unroll
            for (int c = 0; c < NCT; ++c) {
                const float bv = 32 * c + mn < ctot ? cfl[(2 * u + kb) * VBW_FSTR + 32 * c + mn] : 0.f;
                bacc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, bacc[c], 0, 0, 0);
            }
        }
    }
    wave_sync();                                  // the slice is rewritten by the next tile
    }
    if (lmax) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) rmaxv = fmaxf(rmaxv, __shfl_xor(rmaxv, o));
        const unsigned mb = __float_as_uint(rmaxv);                    // (non-negative floats order like their bit patterns; +inf above all)
        if (lane == 0 && mb > *reinterpret_cast<volatile unsigned*>(lmax)) atomicMax(lmax, mb);
    }
    if (gg.basis) {
        // the block's four wavefronts fold their sums through LDS (the basis_mat image is no longer needed), then ONE atomic flush per block
        const int mn = lane & 31, kb = lane >> 5;
        __syncthreads();
        for (int w = 0; w < VBW_WAVES; ++w) {
            if (wv == w) {
#pragma unroll
                for (int c = 0; c < NCT; ++c)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int f = (r & 3) + 8 * (r >> 2) + 4 * kb, ch = 32 * c + mn;
                        if (ch < ctot) bs[f * VBW_BSTR + ch] = w == 0 ? bacc[c][r] : bs[f * VBW_BSTR + ch] + bacc[c][r];
                    }
            }
            __syncthreads();
        }
        for (int o = threadIdx.x; o < F * ctot; o += 64 * VBW_WAVES) {
            const int f = o / ctot, ch = o % ctot;
            const float v = bs[f * VBW_BSTR + ch];
            if (v != 0.f) unsafeAtomicAdd(gg.basis + o, v);
        }
    }
}

// Persistent blocks of the scatter's main kernel.  The 96-channel MFMA instantiation keeps three blocks per CU: exactly that many blocks
// (768 on the 256 CUs of an MI355X), each walking its share of the tiles, measured best -- 0.98 / 0.79 ms per 2^19 samples (rays along z /
// oblique) against 1.02 / 0.82 with 3072 blocks, 1.14 / 0.94 with 1024 (a ragged last round) and 1.07 / 0.97 with 512: every block pays
// for its basis_mat column and flushes its basis_mat gradient (192 atomic requests) once.
static long scatter_blocks_cap(bool three_per_cu) {
    if (!three_per_cu) return 3072;
    const int cus = device_cus(0);
    return cus ? 3L * cus : 3072;
}

// HYBRID: plane taps by direct atomics here, line taps left as rows + tap records (rows_l, ltap) for k_scatter_lines; else every tap here
template <bool HYBRID>
static int launch_sample_bwd_block(const GridParams& g, const float* pts, long n, const float* d_out, int d_stride, int d_col, const GridGrads& gg,
                                   float* d_pts, float* rows_l, LTap* ltap, hipStream_t st) {
    if (g.app_dim > VSB_MAXF) return fail(EVD_E_INVALID, "evd_voxel_sample_bwd: app_dim %d > %d", g.app_dim, VSB_MAXF);
    const long tiles = cdiv(n, VS_SAMPLES);
    const bool mm = g.app_dim == 32 && (g.n_comp[0] + g.n_comp[1] + g.n_comp[2]) % 32 == 0;
    const int ct = g.n_comp[0] + g.n_comp[1] + g.n_comp[2];
    const long cap = scatter_blocks_cap(mm && ct <= 96);
    const unsigned blocks = (unsigned)(tiles < cap ? tiles : cap);
    if (mm && ct <= 96) k_voxel_sample_bwd<HYBRID, true, 96><<<blocks, 256, 0, st>>>(g, pts, n, d_out, d_stride, d_col, gg, d_pts, rows_l, ltap);
    else if (mm) k_voxel_sample_bwd<HYBRID, true, VS_MAXC><<<blocks, 256, 0, st>>>(g, pts, n, d_out, d_stride, d_col, gg, d_pts, rows_l, ltap);
    else k_voxel_sample_bwd<HYBRID, false, VS_MAXC><<<blocks, 256, 0, st>>>(g, pts, n, d_out, d_stride, d_col, gg, d_pts, rows_l, ltap);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int launch_voxel_sample_bwd(const GridParams& g, const float* pts, long n, const float* d_out, int d_stride, int d_col, const GridGrads& gg,
                            float* d_pts, hipStream_t st) {
    return launch_sample_bwd_block<false>(g, pts, n, d_out, d_stride, d_col, gg, d_pts, nullptr, nullptr, st);
}

int launch_voxel_sample_bwd_planes(const GridParams& g, const float* pts, long n, const float* d_out, int d_stride, int d_col, const GridGrads& gg,
                                   float* d_pts, float* rows_l, LTap* ltap, hipStream_t st) {
    return launch_sample_bwd_block<true>(g, pts, n, d_out, d_stride, d_col, gg, d_pts, rows_l, ltap, st);
}

// the wavefront-autonomous form (k_voxel_sample_bwd_w); the caller runs k_scatter_lines on rows_l / ltap afterwards
bool voxel_sample_bwd_w_ok(const GridParams& g) {
    const int ct = g.n_comp[0] + g.n_comp[1] + g.n_comp[2];
    auto okc = [](int c) { return c == 8 || c == 16 || c == 32 || c == 64; };
    const long pmax = (long)g.grid[0] * g.grid[1] > (long)g.grid[0] * g.grid[2] ? (long)g.grid[0] * g.grid[1] : (long)g.grid[0] * g.grid[2];
    const long pm2 = (long)g.grid[1] * g.grid[2] > pmax ? (long)g.grid[1] * g.grid[2] : pmax;
    // (ct % 32: a sample's 8-channel groups are whole quads of lanes -- the point gradient's quad sums; other widths take the block-cooperative kernel)
    return g.app_dim >= 4 && g.app_dim <= 32 && g.app_dim % 4 == 0 && ct % 32 == 0 && ct <= 96 && okc(g.n_comp[0]) && okc(g.n_comp[1]) && okc(g.n_comp[2]) &&
           pm2 * 64 < (1L << 31) && g.app_act == EVD_ACT_NONE;
}
int launch_voxel_sample_bwd_w(const GridParams& g, const float* pts, long n, const float* d_out, int d_stride, int d_col, const GridGrads& gg,
                              float* d_pts, float* rows_l, LTap* ltap, unsigned* lmax, bool half_grids, hipStream_t st) {
    const int cus = device_cus();
    const long tiles = cdiv(n, (long)VBW_SAMPLES * VBW_WAVES);
    // persistent workgroups with the basis gradient in registers: two per CU (the LDS slices allow no more)
    const unsigned blocks = (unsigned)(tiles < 2L * cus ? tiles : 2L * cus);
#define EVD_VBW(DP, H) { EVD_SET_MAX_LDS((&k_voxel_sample_bwd_w<DP, H>), VBW_LDS); \
        k_voxel_sample_bwd_w<DP, H><<<blocks, 64 * VBW_WAVES, VBW_LDS, st>>>(g, pts, n, d_out, d_stride, d_col, gg, d_pts, rows_l, ltap, lmax); }
    // the re-gather reads the float16 copies of the grids where the forward did
    bool have_h = true;
    for (int i = 0; i < 3; ++i) have_h = have_h && g.plane_h[i] && g.line_h[i];
    if (half_grids && have_h) {
        if (d_pts) EVD_VBW(true, true)
        else EVD_VBW(false, true)
    } else {
        if (d_pts) EVD_VBW(true, false)
        else EVD_VBW(false, false)
    }
#undef EVD_VBW
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

}  // namespace evd
