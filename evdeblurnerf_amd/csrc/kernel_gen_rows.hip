// The per-layer kernels on float32 rows (gen_rows.h): forward Linear + bias + ReLU, dgrad, wgrad + fixed-order reduction, the two encodings.
// reference: the autograd graph of networks/nerf.py:131-162, networks/pdrf/voxnerf.py:210-254, networks/dpnerf/awp.py:98-100 (nn.Linear + ReLU
// layers), networks/embedding.py:88-98.
#include "gen_rows.h"
#include "mlp_device.h"

namespace evd {

// Every matrix product is v_mfma_f32_32x32x2f32: lane l gives A[l & 31][l >> 5] and B[l >> 5][l & 31]; register r of the
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

// Forward layer.  A = the weight block (row = output column m, summed index k), B = the input rows (column = sample).  One wavefront owns
// 32 samples and keeps its half of their input rows in registers: slot t of lane half hh is k = 2 t + hh, so step t adds k = 2 t and
// 2 t + 1 -- k ascends, whatever the grid.  The workgroup's four wavefronts share the [32, K] weight block of 32 output columns: read in
// place (K contiguous floats per row) into LDS once, rows of 33 floats so that both the transposing write and the A-operand read are
// conflict-free.
template <int K>
__global__ __launch_bounds__(256, 2) void k_gen_linear_relu(const GenLinear a) {
    constexpr int LD = 33;
    __shared__ float wt[K * LD];            // wt[k * LD + j]: Wm[m0 + j, k]
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 31, hh = lane >> 5;
    const long s = ((long)blockIdx.x * 4 + (tid >> 6)) * 32 + n;
    const bool valid = s < a.nsamp;         // every thread stays for the barriers; a row past nsamp is neither read nor written
    float x[K / 2];
    const float* xrow = a.X + (valid ? s : 0) * a.ldx;
#pragma unroll
    for (int i = 0; i < K / 8; ++i) {
        const f32x4 lo = *reinterpret_cast<const f32x4*>(xrow + 8 * i), hi = *reinterpret_cast<const f32x4*>(xrow + 8 * i + 4);
        x[4 * i] = hh ? lo[1] : lo[0];
        x[4 * i + 1] = hh ? lo[3] : lo[2];
        x[4 * i + 2] = hh ? hi[1] : hi[0];
        x[4 * i + 3] = hh ? hi[3] : hi[2];
        if (!valid) x[4 * i] = x[4 * i + 1] = x[4 * i + 2] = x[4 * i + 3] = 0.f;
    }
    for (int m0 = 0; m0 < AWPG_W; m0 += 32) {
        for (int idx = tid; idx < 32 * K; idx += 256) {
            const int j = idx / K, k = idx % K;
            wt[k * LD + j] = a.Wm[(size_t)(m0 + j) * K + k];
        }
        __syncthreads();
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int t = 0; t < K / 2; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wt[(2 * t + hh) * LD + n], x[t], acc, 0, 0, 0);
        __syncthreads();                    // the block is free for the next 32 columns
        if (valid) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int m = m0 + 8 * q + 4 * hh;
                const f32x4 b = *reinterpret_cast<const f32x4*>(a.bias + m);
                f32x4 y;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float v = b[e] + acc[4 * q + e];
                    y[e] = v > 0.f ? v : 0.f;
                }
                *reinterpret_cast<f32x4*>(a.out + s * AWPG_W + m) = y;
                if (a.out2) *reinterpret_cast<f32x4*>(a.out2 + s * AWPG_W + m) = y;
            }
        }
    }
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

int launch_gen_linear_relu(int K, const GenLinear& a, hipStream_t st) {
    const dim3 grid((unsigned)cdiv(a.nsamp, 128)), block(256);
    switch (K) {
    case 64: hipLaunchKernelGGL(k_gen_linear_relu<64>, grid, block, 0, st, a); break;
    case 128: hipLaunchKernelGGL(k_gen_linear_relu<128>, grid, block, 0, st, a); break;
    case 256: hipLaunchKernelGGL(k_gen_linear_relu<256>, grid, block, 0, st, a); break;
    default: return fail(EVD_E_INVALID, "evd_awp_embed_f32_forward: no kernel for %d input columns (built: 64, 128, 256)", K);
    }
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

}  // namespace evd
