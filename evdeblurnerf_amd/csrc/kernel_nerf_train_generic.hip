// Generic NeRF-mode training kernels (nerf_train_generic.h): forward that keeps float32 activation rows, and the per-layer backward
// (dgrad, wgrad + fixed-order reduction, the two encodings) in exact float32 on the matrix cores.
// reference: the autograd graph of networks/nerf.py:46-72 (mlpforward), :131-162 (eval), networks/embedding.py:88-98.
#include "nerf_train_generic.h"
#include "mlp_device.h"

namespace evd {

// ---------------------------------------------------------------------------------------------------------------------
// Forward: k_nerf_mlp_generic<EVD_PREC_F16X3, W, VKS> (kernel_nerf_mlp.hip) -- the same stream, the same layer<> calls in the same
// order, hence the same raw bit for bit -- with every layer's output written as a float32 row of the store (layer<>'s feat_row).
// A kernel of its own and not a switch in k_nerf_mlp_generic: the inference kernels' code objects stay what they were.
// PDH: where the point encoding's k-steps sit in the skip layer, [h_0 .. h_{PDH-1} | pe | h_PDH .. h_{KS-1}] (nerf_streams.h nerf_layers).  0: the
// generic stream; KS - 2: evd_nerf::stream_pd, the pipelined kernel's order of additions, for the pipelined network's forward with a feature.
template <int W, int VKS, int PDH = 0>
__global__ __launch_bounds__(mlp_threads(EVD_PREC_F16X3), 1) void k_nerf_train_fwd_generic(const MlpParams p) {
    constexpr int PREC = EVD_PREC_F16X3;
    typedef Ops<PREC> O;
    typedef typename O::B B;
    constexpr int NT = mlp_threads(PREC);
    constexpr int T = W / 32, KS = W / 16;
    constexpr int FPC = Stream<PREC>::FPC;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 31, h = lane >> 5;
    const long s = (long)blockIdx.x * (NT / 2) + wave * 32 + n;
    const bool valid = s < p.nsamp;
    const long sc = valid ? s : p.nsamp - 1;
    const long ray = sc / p.S;
    const float* rb = p.ray_batch + ray * p.ncol;
    const float zv = p.z[sc];
    float pts[3], vd[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        pts[c] = __fadd_rn(rb[c], __fmul_rn(rb[3 + c], zv));   // renderer.py:180
        vd[c] = rb[8 + c];
    }
    const GenStore gs(p.nsamp, p.D, W);
    float* const store = reinterpret_cast<float*>(p.act);
    if (valid) {        // the encodings' inputs: lane half 0 the position, half 1 the direction
        const f32x4 v = h ? f32x4{vd[0], vd[1], vd[2], 0.f} : f32x4{pts[0], pts[1], pts[2], 0.f};
        *reinterpret_cast<f32x4*>(store + gs.in() + s * 8 + 4 * h) = v;
    }

    float* bias = stage_bias<PREC>(smem, p.bias, p.nbias, tid);
    B* stash = reinterpret_cast<B*>(smem + MlpLds<PREC>::RING + MlpLds<PREC>::BIAS_FLOATS * 4 + wave * MlpLds<PREC>::STASH_PER_WAVE) + lane;
    B act[KS], nxt[KS];
    {
        B in_pe[PE_KS];
        encode_b_rt<PREC, PE_KS>(pts, h, p.pe_l, in_pe);
#pragma unroll
        for (int j = 0; j < PE_KS; ++j) stash[j * 64] = in_pe[j];
    }
    Stream<PREC> st;
    st.start(p.wstream, smem, p.nchunks, tid);
    float* hrow = valid ? store + gs.h(0) + s * W : nullptr;       // row s of H_0; H_l is nsp * W floats further per layer
    const long hstep = gs.nsp * W;
    {
        B in_pe[PE_KS];
#pragma unroll
        for (int j = 0; j < PE_KS; ++j) in_pe[j] = stash[j * 64];
        layer<PREC, PE_KS, T, true, OUT_B, 0, true>(st, in_pe, nxt, nullptr, bias, lane, hrow, W);
    }
    bias += T * 32;
#pragma unroll
    for (int j = 0; j < KS; ++j) act[j] = nxt[j];

#pragma nounroll
    for (int l = 1; l < p.D; ++l) {
        if (hrow) hrow += hstep;
        if (l - 1 == p.skip) {      // h = cat([input_pts, h]) feeds this layer (nerf.py:137-138)
            B wide[PE_KS + KS];
#pragma unroll
            for (int j = 0; j < PDH; ++j) wide[j] = act[j];
#pragma unroll
            for (int j = 0; j < PE_KS; ++j) wide[PDH + j] = stash[j * 64];
#pragma unroll
            for (int j = PDH; j < KS; ++j) wide[PE_KS + j] = act[j];
            layer<PREC, PE_KS + KS, T, true, OUT_B, 0, true>(st, wide, nxt, nullptr, bias, lane, hrow, W);
        } else {
            layer<PREC, KS, T, true, OUT_B, 0, true>(st, act, nxt, nullptr, bias, lane, hrow, W);
        }
        bias += T * 32;
#pragma unroll
        for (int j = 0; j < KS; ++j) act[j] = nxt[j];
    }

    // heads: alpha_linear (1 tile), feature_linear, views_linears.0 on cat([feature, dirs]), rgb_linear (nerf.py:144-157)
    constexpr int F_ALPHA = KS, F_FEAT = T * KS, F_VIEWS = (T / 2) * (KS + VKS);
    constexpr int OFF_FEAT = F_ALPHA % FPC, OFF_VIEWS = (F_ALPHA + F_FEAT) % FPC, OFF_RGB = (F_ALPHA + F_FEAT + F_VIEWS) % FPC;
    float araw[16], rraw[16];
    layer<PREC, KS, 1, false, OUT_F32, 0, false>(st, act, nullptr, araw, bias, lane, nullptr, W);
    bias += 32;
    layer<PREC, KS, T, false, OUT_B, OFF_FEAT, false>(st, act, nxt, nullptr, bias, lane, valid ? store + gs.f() + s * W : nullptr, W);
    bias += T * 32;
    {
        B vin[KS + VKS];
#pragma unroll
        for (int j = 0; j < KS; ++j) vin[j] = nxt[j];
        {
            B in_dir[VKS];
            encode_b_rt<PREC, VKS>(vd, h, p.pe_lv, in_dir);
#pragma unroll
            for (int j = 0; j < VKS; ++j) vin[KS + j] = in_dir[j];
        }
        layer<PREC, KS + VKS, T / 2, true, OUT_B, OFF_VIEWS, false>(st, vin, act, nullptr, bias, lane, valid ? store + gs.hv() + s * (W / 2) : nullptr, W);
        bias += (T / 2) * 32;
    }
    {
        B hin[KS / 2];
#pragma unroll
        for (int j = 0; j < KS / 2; ++j) hin[j] = act[j];
        layer<PREC, KS / 2, 1, false, OUT_F32, OFF_RGB, true>(st, hin, nullptr, rraw, bias, lane, nullptr, W);
    }
    if (h == 0 && valid) {
        const f32x4 o = {rraw[0], rraw[1], rraw[2], araw[0]};   // cat([rgb, alpha]) nerf.py:157
        *reinterpret_cast<f32x4*>(p.raw + s * 4) = o;
    }
}

template <int W, int VKS, int PDH = 0>
static int launch_fwd(const MlpParams& p, hipStream_t st) {
    constexpr int PREC = EVD_PREC_F16X3, NT = mlp_threads(PREC);
    const long blocks = cdiv(p.nsamp, NT / 2);
    const size_t lds = MlpLds<PREC>::TOTAL;
    EVD_SET_MAX_LDS((&k_nerf_train_fwd_generic<W, VKS, PDH>), lds);
    if (p.nbias > MlpLds<PREC>::BIAS_FLOATS) return fail(EVD_E_INVALID, "evd_nerf_mlp_train: %d bias floats exceed the LDS bias block", p.nbias);
    hipLaunchKernelGGL((k_nerf_train_fwd_generic<W, VKS, PDH>), dim3((unsigned)blocks), dim3(NT), lds, st, p);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int launch_nerf_train_fwd_generic(int W, const MlpParams& p, hipStream_t st, int pdh) {
    const bool widev = pe_ksteps(p.pe_lv) > 2;
    if (pdh) {          // the pipelined network's stream_pd: one shape
        if (W == 256 && !widev && pdh == 14) return launch_fwd<256, 2, 14>(p, st);      // (10, 4): two direction k-steps
        return fail(EVD_E_INVALID, "evd_nerf_mlp_train_feature: no training kernel for the skip layer order %d at width %d", pdh, W);
    }
    if (W == 64) return widev ? launch_fwd<64, 4>(p, st) : launch_fwd<64, 2>(p, st);
    if (W == 128) return widev ? launch_fwd<128, 4>(p, st) : launch_fwd<128, 2>(p, st);
    if (W == 256) return widev ? launch_fwd<256, 4>(p, st) : launch_fwd<256, 2>(p, st);
    return fail(EVD_E_INVALID, "evd_nerf_mlp_train: no generic training kernel for width %d (built: 64, 128, 256)", W);
}

// ---------------------------------------------------------------------------------------------------------------------
// Backward.  Every matrix product is v_mfma_f32_32x32x2f32: lane l gives A[l & 31][l >> 5] and B[l >> 5][l & 31]; register r of the
// result is D[(r & 3) + 8 (r >> 2) + 4 (l >> 5)][l & 31].  The summed index may be dealt to the (step, lane half) slots in any order as
// long as A and B agree, which lets every lane read contiguous floats.

// The two encodings as float32 rows in the reference's column order [x, sin(x f0), cos(x f0), ...] (embedding.py:88-98), zero padded to
// GEN_ENC columns; the values are the forward's (same sin_or_cos, same argument).  thread = one column of one sample, PE(pts) then PE(dirs).
__global__ __launch_bounds__(256) void k_gen_encode(const float* __restrict__ in, long nsamp, int L, int Lv, float* __restrict__ ep, float* __restrict__ ed) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long s = i >> 7;
    if (s >= nsamp) return;
    const int q = (int)(i & 63), which = (int)(i >> 6) & 1;
    const float* x = in + s * 8 + 4 * which;
    const int Lq = which ? Lv : L;
    float y = 0.f;
    if (q < 3) {
        y = x[q];
    } else {
        const int f = (q - 3) / 6, r = (q - 3) % 6;
        if (f < Lq) y = sin_or_cos(x[r % 3] * (float)(1 << f), r / 3);
    }
    (which ? ed : ep)[s * GEN_ENC + q] = y;
}

// d x = d E[x] + sum_f 2^f (cos(2^f x) d E[sin_f] - sin(2^f x) d E[cos_f]), frequencies in ascending order.  thread = one sample.
__global__ __launch_bounds__(256) void k_gen_encode_bwd(const float* __restrict__ enc, const float* __restrict__ denc, long nsamp, int L, float* __restrict__ dx) {
    const long s = (long)blockIdx.x * 256 + threadIdx.x;
    if (s >= nsamp) return;
    const float* e = enc + s * GEN_ENC;
    const float* d = denc + s * GEN_ENC;
    float acc[3] = {d[0], d[1], d[2]};
    for (int f = 0; f < L; ++f) {
        const float sc = (float)(1 << f);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float t = e[3 + 6 * f + 3 + c] * d[3 + 6 * f + c] - e[3 + 6 * f + c] * d[3 + 6 * f + 3 + c];
            acc[c] = acc[c] + sc * t;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) dx[s * 3 + c] = acc[c];
}

// d pre-activation of views_linears.0 from d rgb (rgb_linear has three rows: no matrix core needed).  thread = 4 columns of one sample.
__global__ __launch_bounds__(256) void k_gen_rgb_dgrad(const float* __restrict__ d_raw, const float* __restrict__ rgb_w, const float* __restrict__ hv,
                                                       long nsamp, int H, float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int per = H / 4;
    const long s = i / per;
    if (s >= nsamp) return;
    const int k = (int)(i % per) * 4;
    const f32x4 g = *reinterpret_cast<const f32x4*>(d_raw + s * 4);
    const f32x4 m = *reinterpret_cast<const f32x4*>(hv + s * H + k);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float x = g[0] * rgb_w[k + e] + g[1] * rgb_w[H + k + e] + g[2] * rgb_w[2 * H + k + e];
        o[e] = m[e] > 0.f ? x : 0.f;
    }
    *reinterpret_cast<f32x4*>(out + s * H + k) = o;
}

// out[s, k] = src[s, k] (rows of lds floats), zero where a ReLU mask row is given and mask[s, k] <= 0: the gradient of a feature output
// placed in a gradient plane before the dgrad that adds to it.  thread = 4 columns of one sample.
__global__ __launch_bounds__(256) void k_gen_rows_in(const float* __restrict__ src, long lds, const float* __restrict__ mask, long nsamp, int Wd,
                                                     float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int per = Wd / 4;
    const long s = i / per;
    if (s >= nsamp) return;
    const int k = (int)(i % per) * 4;
    const float* x = src + s * lds + k;
    f32x4 o = {x[0], x[1], x[2], x[3]};
    if (mask) {
        const f32x4 m = *reinterpret_cast<const f32x4*>(mask + s * Wd + k);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = m[e] > 0.f ? o[e] : 0.f;
    }
    *reinterpret_cast<f32x4*>(out + s * Wd + k) = o;
}

struct GenDgrad {
    const float* G; int ldg;            // [nsp, M] d loss / d pre-activation of the layer
    const float* Wm; int ldw, c0, K;    // the layer's weight [M, ldw]; the input columns c0 .. c0 + K - 1
    float* out; int ldo;                // [nsp, ldo] rows, ldo >= K rounded up to 32 (columns >= K: zero)
    const float* mask; int ldm;         // ReLU output rows of the producing layer (gradient passes where > 0), or null
    const float *eg, *ew;               // a second, one-row layer on the same input (alpha_linear): eg[4 s] * ew[k] is added, or null
    int add;                            // 1: out += (the point encoding collects layer 0 and the skip layer, in that fixed order)
    long nsamp;
    int Mv;                             // rows m >= Mv of the weight are not read (zero): a gradient block narrower than the kernel's M
};

// out[s, k] = sum_m G[s, m] W[m, c0 + k].  One wavefront owns 32 samples: its G rows stay in registers (slot (i, e) of lane half hh is
// m = 8 i + 4 hh + e: one 16-byte read per 8 columns).  The workgroup's four wavefronts share the weights: per 32 output columns the
// [M, 32] block is read in place (128 contiguous bytes per 32 threads) into LDS once and read back conflict-free as the A operand.
template <int M>
__global__ __launch_bounds__(256, 2) void k_gen_dgrad(const GenDgrad a) {
    __shared__ float wt[M * 32];            // wt[m * 32 + k]: W[m, c0 + k0 + k], zero for k0 + k >= K
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 31, hh = lane >> 5;
    const long s = ((long)blockIdx.x * 4 + (tid >> 6)) * 32 + n;
    const bool valid = s < a.nsamp;         // every thread stays for the barriers; a row past nsamp is neither read nor written
    f32x4 g[M / 8];
    const float* grow = a.G + (valid ? s : 0) * a.ldg + 4 * hh;
#pragma unroll
    for (int i = 0; i < M / 8; ++i) {
        g[i] = *reinterpret_cast<const f32x4*>(grow + 8 * i);
        if (!valid) g[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const float egs = (a.eg && valid) ? a.eg[s * 4] : 0.f;
    for (int k0 = 0; k0 < a.K; k0 += 32) {
        {
            const int k = tid & 31;
            const bool kin = k0 + k < a.K;
            const float* wcol = a.Wm + a.c0 + (kin ? k0 + k : 0);
#pragma unroll 8
            for (int j = 0; j < M / 8; ++j) {      // 8 reads in flight per thread: two workgroups stay resident per CU at M = 256
                const int m = (tid >> 5) + 8 * j;
                const bool in = kin && m < a.Mv;
                const float w = wcol[in ? (size_t)m * a.ldw : 0];
                wt[m * 32 + k] = in ? w : 0.f;
            }
        }
        __syncthreads();
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int i = 0; i < M / 8; ++i) {
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wt[(8 * i + 4 * hh + e) * 32 + n], g[i][e], acc, 0, 0, 0);
        }
        __syncthreads();                    // the block is free for the next 32 columns
        if (valid) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = k0 + 8 * q + 4 * hh;
                f32x4 x = {acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
                if (a.eg) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) x[e] = x[e] + egs * (k + e < a.K ? a.ew[k + e] : 0.f);
                }
                if (a.mask) {
                    const f32x4 m = *reinterpret_cast<const f32x4*>(a.mask + s * a.ldm + k);
#pragma unroll
                    for (int e = 0; e < 4; ++e) x[e] = m[e] > 0.f ? x[e] : 0.f;
                }
                float* o = a.out + s * a.ldo + k;
                if (a.add) {
                    const f32x4 old = *reinterpret_cast<const f32x4*>(o);
                    x = old + x;
                }
                *reinterpret_cast<f32x4*>(o) = x;
            }
        }
    }
}

struct GenWgrad {
    const float* G; int ldg, M;         // [nsamp, M]
    const float* X; int ldx, K;         // [nsamp, K] the layer's input rows
    float* partial;                     // [nsplit][Mp Kp + Mp]: weight tile sums, then the bias sums
    long nsamp;
    int chunk, nsplit, mt, kt, kg;      // samples per range (a multiple of 8), ranges, 32-row / 32-column tiles, groups of GEN_KB column tiles
    int bias;
};
constexpr int GEN_KB = 4;               // column tiles per wavefront: one G read feeds up to four products

// partial[split][m, k] = sum over the range's samples of G[s, m] X[s, k] (and of G[s, m]: the bias gradient, as a fifth product with
// ones, in the wavefronts of column group 0).  One wavefront = (range, row tile, column group); samples in ascending order.
__global__ __launch_bounds__(256) void k_gen_wgrad(const GenWgrad a) {
    const int lane = threadIdx.x & 63, n = lane & 31, hh = lane >> 5;
    const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int tasks = a.mt * a.kg;
    if (w >= (long)a.nsplit * tasks) return;        // wavefront-uniform
    const int split = (int)(w / tasks), task = (int)(w % tasks), m0 = (task / a.kg) * 32, kt0 = (task % a.kg) * GEN_KB;
    const int nt = a.kt - kt0 < GEN_KB ? a.kt - kt0 : GEN_KB;
    const bool wb = a.bias && kt0 == 0;
    const long s0 = (long)split * a.chunk;
    const long s1 = s0 + a.chunk < a.nsamp ? s0 + a.chunk : a.nsamp;
    const bool m_in = m0 + n < a.M;
    const float* gp = a.G + (m_in ? m0 + n : 0);
    bool kin[GEN_KB];
    const float* xp[GEN_KB];
#pragma unroll
    for (int t = 0; t < GEN_KB; ++t) {
        const int k = (kt0 + t) * 32 + n;
        kin[t] = t < nt && k < a.K;
        xp[t] = a.X + (kin[t] ? k : 0);
    }
    f32x16 acc[GEN_KB], accb;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        accb[r] = 0.f;
#pragma unroll
        for (int t = 0; t < GEN_KB; ++t) acc[t][r] = 0.f;
    }
    for (long sb = s0; sb < s1; sb += 8) {
        float gv[4], xv[GEN_KB][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long s = sb + 2 * u + hh;
            const bool s_in = s < s1;
            const long sr = s_in ? s : s0;
            gv[u] = gp[sr * a.ldg];
            gv[u] = (s_in && m_in) ? gv[u] : 0.f;
#pragma unroll
            for (int t = 0; t < GEN_KB; ++t) {
                if (t < nt) {
                    xv[t][u] = xp[t][sr * a.ldx];
                    xv[t][u] = (s_in && kin[t]) ? xv[t][u] : 0.f;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int t = 0; t < GEN_KB; ++t)
                if (t < nt) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(gv[u], xv[t][u], acc[t], 0, 0, 0);
            if (wb) accb = __builtin_amdgcn_mfma_f32_32x32x2f32(gv[u], 1.f, accb, 0, 0, 0);
        }
    }
    const int Mp = a.mt * 32, Kp = a.kt * 32;
    float* P = a.partial + (size_t)split * ((size_t)Mp * Kp + Mp);
#pragma unroll
    for (int t = 0; t < GEN_KB; ++t) {
        if (t < nt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * hh;
                P[(size_t)m * Kp + (kt0 + t) * 32 + n] = acc[t][r];
            }
        }
    }
    if (wb && n == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) P[(size_t)Mp * Kp + m0 + (r & 3) + 8 * (r >> 2) + 4 * hh] = accb[r];
    }
}

// The ranges' partial sums folded in a fixed order into the nn.Linear block (columns c0 .. c0 + K - 1 of rows of ldw floats) and the bias.
// Workgroup = 32 elements x 8 groups of consecutive ranges: a thread sums its group's ranges in ascending order, then the first group's
// thread adds the eight group sums in ascending order -- the same additions in the same order on every call.
constexpr int GEN_RED_GROUPS = 8;
__global__ __launch_bounds__(256) void k_gen_wreduce(const float* __restrict__ partial, int nsplit, int M, int K, int Mp, int Kp, float* __restrict__ dw, int ldw, int c0,
                                                     float* __restrict__ db, int accumulate) {
    __shared__ float part[GEN_RED_GROUPS][32];
    const int e = threadIdx.x & 31, grp = threadIdx.x >> 5;
    const long i = (long)blockIdx.x * 32 + e;
    const long nw = dw ? (long)M * K : 0;
    const bool in = i < nw + (db ? M : 0);
    const size_t stride = (size_t)Mp * Kp + Mp;
    const float* p = partial;
    float* o = nullptr;
    if (in) {
        if (i < nw) {
            const int m = (int)(i / K), k = (int)(i % K);
            p = partial + (size_t)m * Kp + k;
            o = dw + (size_t)m * ldw + c0 + k;
        } else {
            p = partial + (size_t)Mp * Kp + (i - nw);
            o = db + (i - nw);
        }
    }
    const int per = (nsplit + GEN_RED_GROUPS - 1) / GEN_RED_GROUPS;
    const int sp0 = grp * per, sp1 = sp0 + per < nsplit ? sp0 + per : nsplit;
    float sum = 0.f;
    if (in)
        for (int sp = sp0; sp < sp1; ++sp) sum = sum + p[(size_t)sp * stride];
    part[grp][e] = sum;
    __syncthreads();
    if (grp == 0 && in) {
        float tot = part[0][e];
#pragma unroll
        for (int g = 1; g < GEN_RED_GROUPS; ++g) tot = tot + part[g][e];
        *o = accumulate ? *o + tot : tot;
    }
}

void GenChain::wgrad(const float* G, int ldg, int M, const float* X, int ldx, int K, float* dw, int ldw, int c0, float* db) {
    if (rc || (!dw && !db) || K <= 0) return;
    GenWgrad a;
    a.G = G; a.ldg = ldg; a.M = M; a.X = X; a.ldx = ldx; a.K = K; a.partial = partial; a.nsamp = nsamp;
    a.mt = (M + 31) / 32; a.kt = (K + 31) / 32; a.kg = (a.kt + GEN_KB - 1) / GEN_KB; a.bias = db ? 1 : 0;
    const int Mp = a.mt * 32, Kp = a.kt * 32, tasks = a.mt * a.kg;
    // sample ranges: about 2048 wavefronts in flight, as many as the workspace holds, at least 64 samples each; a function of the
    // shapes alone, so that a repeated call sums in the same order
    long nsplit = cdiv(2048, tasks);
    const long cap = (long)(GEN_WS_FLOATS / ((size_t)Mp * Kp + Mp));
    if (nsplit > cap) nsplit = cap;
    if (nsplit > cdiv(nsamp, 64)) nsplit = cdiv(nsamp, 64);
    if (nsplit < 1) nsplit = 1;
    a.chunk = (int)(cdiv(cdiv(nsamp, nsplit), 8) * 8);
    a.nsplit = (int)cdiv(nsamp, a.chunk);
    hipLaunchKernelGGL(k_gen_wgrad, dim3((unsigned)cdiv((long)a.nsplit * tasks, 4)), dim3(256), 0, st, a);
    if (hipGetLastError() != hipSuccess) { rc = fail(EVD_E_HIP, "%s: wgrad launch failed", who); return; }
    const long ne = (dw ? (long)M * K : 0) + (db ? M : 0);
    hipLaunchKernelGGL(k_gen_wreduce, dim3((unsigned)cdiv(ne, 32)), dim3(256), 0, st, (const float*)partial, a.nsplit, M, K, Mp, Kp, dw, ldw, c0, db,
                       accumulate);
    if (hipGetLastError() != hipSuccess) rc = fail(EVD_E_HIP, "%s: wgrad reduction launch failed", who);
}

void GenChain::dgrad(int M, const float* G, int ldg, const float* Wm, int ldw, int c0, int K, float* out, int ldo, const float* mask, int ldm,
                     const float* eg, const float* ew, int add, int Mv) {
    if (rc || K <= 0) return;
    GenDgrad a;
    a.G = G; a.ldg = ldg; a.Wm = Wm; a.ldw = ldw; a.c0 = c0; a.K = K; a.out = out; a.ldo = ldo; a.mask = mask; a.ldm = ldm;
    a.eg = eg; a.ew = ew; a.add = add; a.nsamp = nsamp; a.Mv = Mv > 0 ? Mv : M;
    const dim3 grid((unsigned)cdiv(nsamp, 128)), block(256);
    switch (M) {
    case 32: hipLaunchKernelGGL(k_gen_dgrad<32>, grid, block, 0, st, a); break;
    case 64: hipLaunchKernelGGL(k_gen_dgrad<64>, grid, block, 0, st, a); break;
    case 128: hipLaunchKernelGGL(k_gen_dgrad<128>, grid, block, 0, st, a); break;
    case 256: hipLaunchKernelGGL(k_gen_dgrad<256>, grid, block, 0, st, a); break;
    default: rc = fail(EVD_E_INVALID, "%s: no dgrad kernel for %d gradient columns", who, M); return;
    }
    if (hipGetLastError() != hipSuccess) rc = fail(EVD_E_HIP, "%s: dgrad launch failed", who);
}

int launch_gen_rows_in(const float* src, long lds, const float* mask, long nsamp, int Wd, float* out, hipStream_t st) {
    hipLaunchKernelGGL(k_gen_rows_in, dim3((unsigned)cdiv(nsamp * (Wd / 4), 256)), dim3(256), 0, st, src, lds, mask, nsamp, Wd, out);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int launch_gen_encode(const float* in, long nsamp, int L, int Lv, float* ep, float* ed, hipStream_t st) {
    hipLaunchKernelGGL(k_gen_encode, dim3((unsigned)cdiv(nsamp * 128, 256)), dim3(256), 0, st, in, nsamp, L, Lv, ep, ed);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int launch_gen_encode_bwd(const float* enc, const float* denc, long nsamp, int L, float* dx, hipStream_t st) {
    hipLaunchKernelGGL(k_gen_encode_bwd, dim3((unsigned)cdiv(nsamp, 256)), dim3(256), 0, st, enc, denc, nsamp, L, dx);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int run_nerf_backward_generic(const GenBwdPlan& b, hipStream_t st) {
    const evd_nerf* net = b.net;
    const int D = net->D, W = net->W, H = W / 2, L = net->multires, Lv = net->multires_views;
    const int IC = 3 * (1 + 2 * L), ICV = 3 * (1 + 2 * Lv);
    const long n = b.nsamp;
    if (!net->params_f32.p) return fail(EVD_E_INVALID, "evd_nerf_mlp_backward: the handle holds no float32 parameters for the generic training path");
    const GenStore gs(n, D, W);
    float* S = b.store;
    const float* P = (const float*)net->params_f32.p;
    auto par = [&](int i) { return P + net->param_off[i]; };
    const float *views_w = par(2 * D), *feature_w = par(2 * D + 2), *alpha_w = par(2 * D + 4), *rgb_w = par(2 * D + 6);
    float *ep = S + gs.enc(0), *ed = S + gs.enc(1), *dep = S + gs.enc(2), *ded = S + gs.enc(3);
    float *g0 = S + gs.g(0), *g1 = S + gs.g(1);
    auto hrow = [&](int l) { return (const float*)(S + gs.h(l)); };
    const float *frow = S + gs.f(), *hv = S + gs.hv();

    if (int rc = launch_gen_encode(S + gs.in(), n, L, Lv, ep, ed, st)) return rc;
    GenChain c{n, b.partial, b.accumulate, st, "evd_nerf_mlp_backward"};

    // rgb_linear on hv (nerf.py:155-156)
    c.wgrad(b.d_raw, 4, 3, hv, H, H, b.grads.rgb_w, H, 0, b.grads.rgb_b);
    hipLaunchKernelGGL(k_gen_rgb_dgrad, dim3((unsigned)cdiv(n * (H / 4), 256)), dim3(256), 0, st, b.d_raw, rgb_w, hv, n, H, g0);
    EVD_LAUNCH_CHECK();
    // views_linears.0 on cat([feature, PE(dirs)]) (nerf.py:151-154); g0 = d its pre-activation [n, H]
    c.wgrad(g0, H, H, frow, W, W, b.grads.views_w, W + ICV, 0, b.grads.views_b);
    c.wgrad(g0, H, H, ed, GEN_ENC, ICV, b.grads.views_w, W + ICV, W, nullptr);
    const bool fg1 = b.d_feature && b.feature_kind == 1, fg2 = b.d_feature && b.feature_kind == 2;
    auto rows_in = [&](const float* mask, float* out) { return launch_gen_rows_in(b.d_feature, b.ldf, mask, n, W, out, st); };
    if (fg1)
        if (int rc = rows_in(nullptr, g1)) return rc;
    c.dgrad(H, g0, H, views_w, W + ICV, 0, W, g1, W, nullptr, 0, nullptr, nullptr, fg1 ? 1 : 0);          // g1 = d feature
    if (b.d_dirs) c.dgrad(H, g0, H, views_w, W + ICV, W, ICV, ded, GEN_ENC, nullptr, 0, nullptr, nullptr, 0);
    // feature_linear and alpha_linear on h_{D-1} (nerf.py:144-150)
    c.wgrad(g1, W, W, hrow(D - 1), W, W, b.grads.feature_w, W, 0, b.grads.feature_b);
    c.wgrad(b.d_raw + 3, 4, 1, hrow(D - 1), W, W, b.grads.alpha_w, W, 0, b.grads.alpha_b);
    if (fg2)
        if (int rc = rows_in(hrow(D - 1), g0)) return rc;
    c.dgrad(W, g1, W, feature_w, W, 0, W, g0, W, hrow(D - 1), W, b.d_raw + 3, alpha_w, fg2 ? 1 : 0);      // g0 = d pre-activation of pts_linears[D-1]
    // the trunk, last layer first; cur = d pre-activation of layer l
    float *cur = g0, *oth = g1;
    int pe_written = 0;
    for (int l = D - 1; l >= 0; --l) {
        const float* wl = par(2 * l);
        if (l == 0) {
            c.wgrad(cur, W, W, ep, GEN_ENC, IC, b.grads.pts_w[0], IC, 0, b.grads.pts_b[0]);
            if (b.d_pts) c.dgrad(W, cur, W, wl, IC, 0, IC, dep, GEN_ENC, nullptr, 0, nullptr, nullptr, pe_written);
            break;
        }
        const bool wide = l - 1 == net->skip;       // the layer reads cat([PE(pts), h_{l-1}]) (nerf.py:137-138)
        const int in = wide ? IC + W : W, hc0 = wide ? IC : 0;
        c.wgrad(cur, W, W, hrow(l - 1), W, W, b.grads.pts_w[l], in, hc0, b.grads.pts_b[l]);
        if (wide) {
            c.wgrad(cur, W, W, ep, GEN_ENC, IC, b.grads.pts_w[l], in, 0, nullptr);
            if (b.d_pts) { c.dgrad(W, cur, W, wl, in, 0, IC, dep, GEN_ENC, nullptr, 0, nullptr, nullptr, 0); pe_written = 1; }
        }
        c.dgrad(W, cur, W, wl, in, hc0, W, oth, W, hrow(l - 1), W, nullptr, nullptr, 0);
        float* t = cur; cur = oth; oth = t;
    }
    if (c.rc) return c.rc;
    if (b.d_pts)
        if (int rc = launch_gen_encode_bwd(ep, dep, n, L, b.d_pts, st)) return rc;
    if (b.d_dirs)
        if (int rc = launch_gen_encode_bwd(ed, ded, n, Lv, b.d_dirs, st)) return rc;
    return EVD_OK;
}

}  // namespace evd
