// Tap geometry of the tri-plane gather (kernel_voxel_sample.hip) and of its backward (kernel_voxel_sample_bwd.hip), and the small device
// helpers both directions use.  The scatter re-derives the forward's interpolation weights bit for bit (the f16 / f16c re-gather relies on
// it): both take them from tap_geometry below, the only place where the formulas are written out.
#pragma once

#include "mlp_device.h"
#include "voxel.h"

namespace evd {

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int VS_SAMPLES = 32;      // samples per 256-thread block of the block-cooperative forms (k_voxel_sample, k_voxel_sample_bwd)
constexpr int VS_MAXC = 128;        // max sum(n_comp)

__device__ __forceinline__ float unnorm(float c, int size) { return __fmul_rn(__fadd_rn(c, 1.f) / 2.f, (float)(size - 1)); }

// pick one of three wave-uniform values by a per-lane index WITHOUT indexing the kernel-argument struct dynamically (that
// turns every g.plane[i] / g.grid[..] into a dependent vector load from the argument buffer in front of the real loads)
template <class V> __device__ __forceinline__ V sel3(int i, V a, V b, V c) { return i == 0 ? a : (i == 1 ? b : c); }

// channel c of the concatenated components -> its component i and the channel c inside that component
struct ChannelOf { int i, c; };
__device__ __forceinline__ ChannelOf channel_component(int c, int c0n, int c1n) {
    int i = 0;
    if (c >= c0n) { c -= c0n; i = 1; if (c >= c1n) { c -= c1n; i = 2; } }
    return {i, c};
}

// One sample in one of its three components (plane i x line i): F.grid_sample(bilinear, zeros, align_corners=True).  The
// interpolation-weight form (w = x - floor x, e = 1 - w) and the tap order follow the ATen CPU kernel, unfused.
struct TapGeom {
    int C, Wp, Hp, Lp;                      // channels of the component; plane width, plane height, line length
    int cx0, cx1, cy0, cy1, cl0, cl1;       // cell indices of the taps, clamped into the grid (an outside tap reads a valid address)
    bool vx0, vx1, vy0, vy1, vl0, vl1;      // ... and whether they were inside (outside = the zero padding)
    float ww, ee, nn, ss, ln, ls;           // fractional position in the plane cell (x: ww, 1 - ww; y: nn, 1 - nn) and in the line cell
};

__device__ __forceinline__ TapGeom tap_geometry(const GridParams& g, const float (&pt)[3], int i) {
    // matMode = [[0,1],[0,2],[1,2]], vecMode = [2,1,0] (voxnerf.py:99-100)
    TapGeom t;
    float xyz[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) xyz[c] = __fsub_rn(__fmul_rn(__fsub_rn(pt[c], g.aabb_min[c]), g.inv[c]), 1.f);   // voxnerf.py:205
    t.C = sel3(i, g.n_comp[0], g.n_comp[1], g.n_comp[2]);
    t.Wp = sel3(i, g.grid[0], g.grid[0], g.grid[1]);          // grid[mat0[i]]
    t.Hp = sel3(i, g.grid[1], g.grid[2], g.grid[2]);          // grid[mat1[i]]
    t.Lp = sel3(i, g.grid[2], g.grid[1], g.grid[0]);          // grid[vec[i]]
    const int Wp = t.Wp, Hp = t.Hp, Lp = t.Lp;
    const float cx = sel3(i, xyz[0], xyz[0], xyz[1]), cy = sel3(i, xyz[1], xyz[2], xyz[2]), cl = sel3(i, xyz[2], xyz[1], xyz[0]);
    const float ix = unnorm(cx, Wp), iy = unnorm(cy, Hp);
    // clamp far-away points before the float -> int conversion (everything beyond one cell outside is zero padding)
    const float fx = fminf(fmaxf(floorf(ix), -2.f), (float)Wp), fy = fminf(fmaxf(floorf(iy), -2.f), (float)Hp);
    t.ww = __fsub_rn(ix, floorf(ix)); t.ee = __fsub_rn(1.f, t.ww); t.nn = __fsub_rn(iy, floorf(iy)); t.ss = __fsub_rn(1.f, t.nn);
    const int x0 = (int)fx, y0 = (int)fy, x1 = x0 + 1, y1 = y0 + 1;
    t.vx0 = x0 >= 0 && x0 < Wp; t.vx1 = x1 >= 0 && x1 < Wp; t.vy0 = y0 >= 0 && y0 < Hp; t.vy1 = y1 >= 0 && y1 < Hp;
    t.cx0 = min(max(x0, 0), Wp - 1); t.cx1 = min(max(x1, 0), Wp - 1); t.cy0 = min(max(y0, 0), Hp - 1); t.cy1 = min(max(y1, 0), Hp - 1);
    const float il = unnorm(cl, Lp);
    const float fl = fminf(fmaxf(floorf(il), -2.f), (float)Lp);
    t.ln = __fsub_rn(il, floorf(il)); t.ls = __fsub_rn(1.f, t.ln);
    const int l0 = (int)fl, l1 = l0 + 1;
    t.cl0 = min(max(l0, 0), Lp - 1); t.cl1 = min(max(l1, 0), Lp - 1);
    t.vl0 = l0 >= 0 && l0 < Lp; t.vl1 = l1 >= 0 && l1 < Lp;
    return t;
}

// What the gathers keep of it per (sample, component): element offsets of channel 0 of the 4 plane taps and the 2 line taps (O = long, or
// int where the dispatch has checked that the grids stay below 2^31 elements) and their interpolation weights, 0 = outside.  Computed ONCE per
// (sample, component) and shared through LDS by the component's channel groups -- the first version recomputed it in every (sample, channel
// group) item: 320 VALU instructions per item, the kernel was VALU-bound (PMC: profiles/r02_pmc_voxel.txt).
template <class O> struct Taps {
    O ip[4], il[2];
    float wp[4], wl[2];
};

// fills the ip / il / wp / wl of any tap record, the offsets computed in A (long or int) and stored as the record keeps them;
// live = false (a sample past n): all weights 0
template <class A, class T> __device__ __forceinline__ void tap_offsets_weights(const TapGeom& t, bool live, T& tp) {
    typedef decltype(+tp.ip[0]) O;
    tp.ip[0] = (O)(((A)t.cy0 * t.Wp + t.cx0) * t.C);
    tp.ip[1] = (O)(((A)t.cy0 * t.Wp + t.cx1) * t.C);
    tp.ip[2] = (O)(((A)t.cy1 * t.Wp + t.cx0) * t.C);
    tp.ip[3] = (O)(((A)t.cy1 * t.Wp + t.cx1) * t.C);
    tp.wp[0] = (live && t.vy0 && t.vx0) ? __fmul_rn(t.ee, t.ss) : 0.f;
    tp.wp[1] = (live && t.vy0 && t.vx1) ? __fmul_rn(t.ww, t.ss) : 0.f;
    tp.wp[2] = (live && t.vy1 && t.vx0) ? __fmul_rn(t.ee, t.nn) : 0.f;
    tp.wp[3] = (live && t.vy1 && t.vx1) ? __fmul_rn(t.ww, t.nn) : 0.f;
    tp.il[0] = (O)((A)t.cl0 * t.C);
    tp.il[1] = (O)((A)t.cl1 * t.C);
    tp.wl[0] = (live && t.vl0) ? t.ls : 0.f;
    tp.wl[1] = (live && t.vl1) ? t.ln : 0.f;
}

// What the point gradient needs on top of that
struct TapGrad {
    float fw, fn, fl;       // fractional positions inside the cell (x, y of the plane; the line)
    float kx, ky, kl;       // d (pixel coordinate) / d (point coordinate) of the three axes the component reads
    int ax, ay, al;         // ... and which point axes those are
    int vm;                 // taps inside the grid: bits 0-3 the plane taps, 4-5 the line taps (a tap can be inside with weight 0); 0 for a dead sample
};

__device__ __forceinline__ TapGrad tap_grad(const GridParams& g, const TapGeom& t, int i, bool live) {
    TapGrad e;
    e.fw = t.ww; e.fn = t.nn; e.fl = t.ln;
    e.kx = 0.5f * (float)(t.Wp - 1) * sel3(i, g.inv[0], g.inv[0], g.inv[1]);
    e.ky = 0.5f * (float)(t.Hp - 1) * sel3(i, g.inv[1], g.inv[2], g.inv[2]);
    e.kl = 0.5f * (float)(t.Lp - 1) * sel3(i, g.inv[2], g.inv[1], g.inv[0]);
    e.ax = sel3(i, 0, 0, 1); e.ay = sel3(i, 1, 2, 2); e.al = sel3(i, 2, 1, 0);
    e.vm = live ? ((t.vy0 && t.vx0) | (t.vy0 && t.vx1) << 1 | (t.vy1 && t.vx0) << 2 | (t.vy1 && t.vx1) << 3 | t.vl0 << 4 | t.vl1 << 5) : 0;
    return e;
}

// ---- a gathered item of 4 channels: the values of its 4 + 2 taps and their weights
struct VsItem {
    f32x4 p[4], l[2];
    float wp[4], wl[2];
};

template <bool HALF>
__device__ __forceinline__ f32x4 vs_load(const float* base32, const _Float16* base16, long idx) {
    if (HALF) return __builtin_convertvector(*reinterpret_cast<const f16x4*>(base16 + idx), f32x4);
    return *reinterpret_cast<const f32x4*>(base32 + idx);
}

// invalid taps contribute exactly nothing (the reference skips them): a zero weight times a finite grid value is 0,
// and 0 added to the running sum changes nothing
__device__ __forceinline__ f32x4 vs_finish(const VsItem& it, f32x4* pv_out = nullptr, f32x4* lv_out = nullptr) {
    f32x4 pv = {0.f, 0.f, 0.f, 0.f}, lv = {0.f, 0.f, 0.f, 0.f}, cf;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int k = 0; k < 4; ++k) pv[k] = it.wp[t] != 0.f ? __fadd_rn(pv[k], __fmul_rn(it.p[t][k], it.wp[t])) : pv[k];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int k = 0; k < 4; ++k) lv[k] = it.wl[t] != 0.f ? __fadd_rn(lv[k], __fmul_rn(it.l[t][k], it.wl[t])) : lv[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) cf[k] = __fmul_rn(pv[k], lv[k]);
    if (pv_out) *pv_out = pv;
    if (lv_out) *lv_out = lv;
    return cf;
}

// ---- the split-float16 matrix products (hi = f16(x), lo = f16(x - hi)) and the float16 re-gather
// Power of two that brings a magnitude m into [2^13, 2^14) (float16's largest binades, so that hi / lo splits of values up to m keep
// 2^-22 of m), and its inverse; m = 0, denormal or tiny: the scale of 2^-113; non-finite m passes through (the scaled values are then
// non-finite as well and so is the product, as in float32).
__device__ __forceinline__ float pow2_scale_f16(float m, float* inv) {
    int E = (int)((__float_as_uint(m) >> 23) & 0xffu);
    E = E < 14 ? 14 : E;
    *inv = __uint_as_float((unsigned)(E - 13) << 23);
    return __uint_as_float((unsigned)(267 - E) << 23);
}
// acc + w x (one float16 of a packed pair) in ONE instruction: v_fma_mix_f32 (op_sel_hi marks the float16 source, op_sel picks its high half);
// hipcc does not form it from fmaf(w, (float)h, acc) here (a conversion + a fused multiply-add: 48 more instructions per gathered item)
template <int HI> __device__ __forceinline__ float fma_mix_f16(float w, unsigned pair, float acc) {
    float d;
    if (HI) asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[0,1,0]" : "=v"(d) : "v"(w), "v"(pair), "v"(acc));
    else asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[0,1,0]" : "=v"(d) : "v"(w), "v"(pair), "v"(acc));
    return d;
}
__device__ __forceinline__ float mul_legacy(float a, float b) {          // a x b with 0 x anything = 0 (v_mul_legacy_f32: VOP3 only, no builtin in this hipcc)
    float d;
    asm("v_mul_legacy_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
    return d;
}

}  // namespace evd
