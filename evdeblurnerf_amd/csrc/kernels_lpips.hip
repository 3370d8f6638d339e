// LPIPS of the test-set pass on the device: compute_img_metric(rgbs, target, 'lpips') (reference utils/metrics.py:92-95, called at
// run_nerf.py:688), i.e. networks/lpips/lpips.py LPIPS(net='alex', version='0.1') in eval mode: the first five convolutions of AlexNet on
// both frames, and per layer the head-weighted squared distance of the channel-normalised features, averaged over the pixels.  The
// reference copies every frame to the host and runs the convolutions on the CPU; here everything stays on the caller's stream.  The
// weights are the caller's (evd_lpips_create); float32 features, float64 from the normalisation on.
//   k_lpips_conv<FIRST>   implicit GEMM on v_mfma_f32_32x32x2_f32 (exact float32 products) over channel-last activations [2 B, h, w, C]: the
//                         predicted and the target frames of the whole batch in one launch, M = 2 B ho wo rows (one per output pixel),
//                         N = Cout, K = (ky, kx, c) with c fastest, so that a K tile of 32 is 128 contiguous bytes of one tap.  Weights are
//                         packed once to [Kpad, Cout].  A workgroup of 4 wavefronts owns a 128 x 64 tile, a wavefront 32 rows x 64 columns
//                         (two accumulators: one A read feeds two MFMAs).  Zero padding and the M edge are predicates on the A load.  The
//                         next K tile's global loads are issued before the current tile's MFMAs.  A K tile is summed from zero and then
//                         added to the running accumulator (blocked summation: the chain a rounding error travels through is
//                         16 + K / 32 additions, not K / 2).  Epilogue: + bias, ReLU.  FIRST (conv1, Cin 3, K 363): reads the caller's
//                         [B, H, W, 3] frames, pred then target, and applies clamp(2 x - 1, -1, 1) (utils/metrics.py:48-49) and the
//                         scaling layer (x - shift) / scale (lpips.py:245-252) on load, element by element.
//   k_lpips_pool          MaxPool(3, stride 2, floor) in front of conv2 and conv3, channel-last, float4.
//   k_lpips_dist          per layer: a wavefront per pixel, n = sqrt(sum_c f^2) for both frames and
//                         d = sum_c lin_c (f0_c / (n0 + 1e-10) - f1_c / (n1 + 1e-10))^2 in float64 by butterflies; a workgroup sums its 64
//                         pixels in a fixed order into one float64 partial.
//   k_lpips_finish        one workgroup: a wavefront per (image, layer) sums that pair's partials in a fixed order and divides by the pixel
//                         count; the five terms are added layer by layer, the batch mean image by image.
// No floating-point atomics: two runs give the same bits, an image's value does not depend on the rest of the batch, and since every
// output element of a convolution is the same instruction sequence wherever it lies, identical frames give identical features and exactly 0.
#include <algorithm>

#include "evd_common.h"

namespace evd {

typedef float lp_f32x16 __attribute__((ext_vector_type(16)));

constexpr int LP_L = EVD_LPIPS_LAYERS;
constexpr int LP_BM = 128, LP_BN = 64, LP_KT = 32, LP_THREADS = 256;
constexpr int LP_ALD = LP_KT + 1;        // A tile rows padded: lane r of a wavefront reads row r, 33 r mod 64 are distinct banks
constexpr int LP_BLD = LP_BN + 32;       // B tile rows: the two lane halves read rows k and k + 1, 96 floats apart = the other 32 banks
constexpr int LP_DPIX = 64;              // pixels per workgroup of k_lpips_dist (16 per wavefront)
constexpr int LP_FINISH_THREADS = 1024;
static_assert(LP_THREADS == 2 * LP_BM && LP_THREADS * 8 == LP_KT * LP_BN && LP_KT == 32, "load mapping: 16 A values and 8 B values per thread");

// AlexNet features[0:12] (torchvision): conv k / stride / pad, Cin -> Cout; a MaxPool(3, 2) in front of layers 1 and 2
constexpr int LP_KS[LP_L] = {11, 5, 3, 3, 3}, LP_STRIDE[LP_L] = {4, 1, 1, 1, 1}, LP_PAD[LP_L] = {2, 2, 1, 1, 1};
constexpr int LP_CIN[LP_L] = {3, 64, 192, 384, 256}, LP_COUT[LP_L] = {64, 192, 384, 256, 256};
constexpr bool LP_POOL[LP_L] = {false, true, true, false, false};

struct LpConv {
    int Hin, Win, Cin, Hout, Wout, Cout, ks, stride, pad, K, nkt;
    int M;                               // 2 B Hout Wout
};
struct LpScale {
    float shift[3], scale[3];
};
struct LpFinish {
    long off[LP_L];                      // the layer's first partial
    int chunks[LP_L];                    // partials per image
    int hw[LP_L];                        // pixels per image
};

// (im * 2 - 1).clamp(-1, 1), then the scaling layer, in float32 as the reference computes them; NaN stays NaN
__device__ __forceinline__ float lp_map(float v, float shift, float scale) {
    v = v * 2.f - 1.f;
    v = v < -1.f ? -1.f : (v > 1.f ? 1.f : v);
    return (v - shift) / scale;
}

__device__ __forceinline__ double lp_wave_sum(double v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// in: FIRST ? pred [B, H, W, 3] : activations [2 B, Hin, Win, Cin]; in2: target (FIRST only); wpk [nkt * 32, Cout]; out [M, Cout]
template <bool FIRST>
__global__ __launch_bounds__(LP_THREADS) void k_lpips_conv(const float* __restrict__ in, const float* __restrict__ in2, int B,
                                                          const float* __restrict__ wpk, const float* __restrict__ bias, LpConv g, LpScale sc,
                                                          float* __restrict__ out) {
    __shared__ float s_a[LP_BM][LP_ALD];
    __shared__ float s_b[LP_KT][LP_BLD];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int m0 = blockIdx.x * LP_BM, n0 = blockIdx.y * LP_BN;

    // the A row this thread stages: output pixel m -> image, top-left input coordinate
    const int arow = tid >> 1, akq = (tid & 1) * 16;
    const int am = m0 + arow;
    const bool arow_ok = am < g.M;
    int iy0 = 0, ix0 = 0;
    const float* img = in;
    {
        const int mm = arow_ok ? am : 0;
        const int hw = g.Hout * g.Wout;
        const int n = mm / hw, p = mm - n * hw;
        const int oy = p / g.Wout, ox = p - oy * g.Wout;
        iy0 = oy * g.stride - g.pad;
        ix0 = ox * g.stride - g.pad;
        const long per = (long)g.Hin * g.Win * g.Cin;
        img = FIRST ? (n < B ? in + n * per : in2 + (n - B) * per) : in + n * per;
    }
    const int bk = tid >> 3, bn = (tid & 7) * 8;
    const float* wcol = wpk + n0 + bn;

    float ra[16];
    float4 rb[2];
    auto load_tile = [&](int kt) {
        const int k0 = kt * LP_KT;
        if constexpr (FIRST) {           // Cin 3: k = (ky * 11 + kx) * 3 + c, decoded per element; k >= K reads as 0
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int k = k0 + akq + j;
                const int ky = k / 33, r = k - ky * 33, kx = r / 3, c = r - kx * 3;
                const int iy = iy0 + ky, ix = ix0 + kx;
                const bool ok = arow_ok && k < g.K && iy >= 0 && iy < g.Hin && ix >= 0 && ix < g.Win;
                ra[j] = ok ? lp_map(img[(iy * g.Win + ix) * 3 + c], sc.shift[c], sc.scale[c]) : 0.f;
            }
        } else {                         // Cin a multiple of 32: the tile lies inside one tap, 16 contiguous floats per thread
            const int tap = k0 / g.Cin, c0 = k0 - tap * g.Cin + akq;
            const int ky = tap / g.ks, kx = tap - ky * g.ks;
            const int iy = iy0 + ky, ix = ix0 + kx;
            const bool ok = arow_ok && iy >= 0 && iy < g.Hin && ix >= 0 && ix < g.Win;
            if (ok) {
                const float4* p = reinterpret_cast<const float4*>(img + ((long)iy * g.Win + ix) * g.Cin + c0);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 v = p[q];
                    ra[4 * q] = v.x;
                    ra[4 * q + 1] = v.y;
                    ra[4 * q + 2] = v.z;
                    ra[4 * q + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 16; ++j) ra[j] = 0.f;
            }
        }
        const float4* q = reinterpret_cast<const float4*>(wcol + (long)(k0 + bk) * g.Cout);
        rb[0] = q[0];
        rb[1] = q[1];
    };

    lp_f32x16 acc0, acc1;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc0[i] = acc1[i] = 0.f;
    const int r = lane & 31, h = lane >> 5;

    load_tile(0);
    for (int kt = 0; kt < g.nkt; ++kt) {
#pragma unroll
        for (int j = 0; j < 16; ++j) s_a[arow][akq + j] = ra[j];
        *reinterpret_cast<float4*>(&s_b[bk][bn]) = rb[0];
        *reinterpret_cast<float4*>(&s_b[bk][bn + 4]) = rb[1];
        __syncthreads();
        if (kt + 1 < g.nkt) load_tile(kt + 1);
        lp_f32x16 t0, t1;
#pragma unroll
        for (int i = 0; i < 16; ++i) t0[i] = t1[i] = 0.f;
#pragma unroll
        for (int kk = 0; kk < LP_KT / 2; ++kk) {
            const int k = 2 * kk + h;
            const float a = s_a[wave * 32 + r][k];
            const float b0 = s_b[k][r], b1 = s_b[k][32 + r];
            t0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, t0, 0, 0, 0);
            t1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, t1, 0, 0, 0);
        }
        acc0 += t0;
        acc1 += t1;
        __syncthreads();
    }

    // C layout: column = lane & 31, row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5)
    const float bias0 = bias[n0 + r], bias1 = bias[n0 + 32 + r];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int m = m0 + wave * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
        if (m < g.M) {
            float* o = out + (long)m * g.Cout + n0 + r;
            o[0] = act(EVD_ACT_RELU, acc0[i] + bias0);
            o[32] = act(EVD_ACT_RELU, acc1[i] + bias1);
        }
    }
}

// MaxPool2d(3, stride 2), floor: every window lies inside the map.  x [N, Hin, Win, C] -> y [N, Ho, Wo, C], C a multiple of 4; NaN wins
__global__ __launch_bounds__(256) void k_lpips_pool(const float* __restrict__ x, int Hin, int Win, int C, int Ho, int Wo, long total4,
                                                    float* __restrict__ y) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= total4) return;
    const int c4 = C >> 2;
    const int c = (int)(i % c4);
    long p = i / c4;
    const int ox = (int)(p % Wo);
    p /= Wo;
    const int oy = (int)(p % Ho);
    const long n = p / Ho;
    const float4* src = reinterpret_cast<const float4*>(x) + ((n * Hin + 2 * oy) * Win + 2 * ox) * c4 + c;
    float4 m = src[0];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const float4 v = src[((long)dy * Win + dx) * c4];
            m.x = (v.x > m.x || v.x != v.x) ? v.x : m.x;
            m.y = (v.y > m.y || v.y != v.y) ? v.y : m.y;
            m.z = (v.z > m.z || v.z != v.z) ? v.z : m.z;
            m.w = (v.w > m.w || v.w != v.w) ? v.w : m.w;
        }
    reinterpret_cast<float4*>(y)[i] = m;
}

// feat [2 B, hw, C]: image b's predicted frame is row block b, its target row block B + b.  grid (chunks, B); partials [B, chunks]
__global__ __launch_bounds__(256) void k_lpips_dist(const float* __restrict__ feat, const float* __restrict__ lin, int B, int hw, int C,
                                                    double* __restrict__ partials) {
    __shared__ double s_red[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.y;
    double acc = 0.0;                    // the same value in every lane
    for (int i = 0; i < LP_DPIX / 4; ++i) {
        const int p = blockIdx.x * LP_DPIX + wave * (LP_DPIX / 4) + i;
        if (p >= hw) break;
        const float* f0 = feat + ((long)b * hw + p) * C;
        const float* f1 = feat + ((long)(B + b) * hw + p) * C;
        double s0 = 0.0, s1 = 0.0;
        for (int c = lane; c < C; c += 64) {
            const double a = (double)f0[c], t = (double)f1[c];
            s0 += a * a;
            s1 += t * t;
        }
        const double d0 = sqrt(lp_wave_sum(s0)) + 1e-10, d1 = sqrt(lp_wave_sum(s1)) + 1e-10;
        double d = 0.0;
        for (int c = lane; c < C; c += 64) {
            const double e = (double)f0[c] / d0 - (double)f1[c] / d1;       // all-zero features: 0 / 1e-10 = 0
            d += (double)lin[c] * (e * e);
        }
        acc += lp_wave_sum(d);
    }
    if (lane == 0) s_red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[(long)b * gridDim.x + blockIdx.x] = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
}

// out: value [B], mean, term [B, 5]
__global__ __launch_bounds__(LP_FINISH_THREADS) void k_lpips_finish(const double* __restrict__ partials, LpFinish f, int B, double* __restrict__ out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double* term = out + B + 1;
    for (int it = wave; it < B * LP_L; it += LP_FINISH_THREADS / 64) {
        const int b = it / LP_L, l = it - b * LP_L;
        const double* p = partials + f.off[l] + (long)b * f.chunks[l];
        double s = 0.0;
        for (int t = lane; t < f.chunks[l]; t += 64) s += p[t];
        s = lp_wave_sum(s);
        if (lane == 0) term[it] = s / (double)f.hw[l];
    }
    __syncthreads();
    for (int b = threadIdx.x; b < B; b += LP_FINISH_THREADS) {      // val = res[0] + res[1] + ... (lpips.py forward)
        double v = term[b * LP_L];
        for (int l = 1; l < LP_L; ++l) v += term[b * LP_L + l];
        out[b] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {              // sum(values) / len(values), image by image (utils/metrics.py:100)
        double s = 0.0;
        for (int b = 0; b < B; ++b) s += out[b];
        out[B] = s / (double)B;
    }
}

// sizes of every stage for B frames of H x W
struct LpPlan {
    LpConv conv[LP_L];
    int pool_h[LP_L], pool_w[LP_L];      // the pooled map in front of layers 1, 2
    LpFinish fin;
    long n_partials;
    size_t buf_floats;                   // each of the two activation buffers
};

static bool lp_plan(int B, int H, int W, LpPlan* pl) {
    if (B < 1 || H < EVD_LPIPS_MIN_SIDE || W < EVD_LPIPS_MIN_SIDE || (long)H * W * 3 >= (1L << 31)) return false;
    int h = H, w = W;
    long np = 0;
    size_t buf = 0;
    for (int l = 0; l < LP_L; ++l) {
        if (LP_POOL[l]) {
            h = (h - 3) / 2 + 1;
            w = (w - 3) / 2 + 1;
            pl->pool_h[l] = h;
            pl->pool_w[l] = w;
            buf = std::max(buf, (size_t)2 * B * h * w * LP_CIN[l]);
        } else {
            pl->pool_h[l] = pl->pool_w[l] = 0;
        }
        LpConv& c = pl->conv[l];
        c.Hin = h;
        c.Win = w;
        c.Cin = LP_CIN[l];
        c.ks = LP_KS[l];
        c.stride = LP_STRIDE[l];
        c.pad = LP_PAD[l];
        c.Cout = LP_COUT[l];
        c.Hout = (h + 2 * c.pad - c.ks) / c.stride + 1;
        c.Wout = (w + 2 * c.pad - c.ks) / c.stride + 1;
        c.K = c.ks * c.ks * c.Cin;
        c.nkt = (int)cdiv(c.K, LP_KT);
        const long M = 2L * B * c.Hout * c.Wout;
        if (M >= (1L << 31) - LP_BM) return false;
        c.M = (int)M;
        h = c.Hout;
        w = c.Wout;
        buf = std::max(buf, (size_t)M * c.Cout);
        pl->fin.hw[l] = h * w;
        pl->fin.chunks[l] = (int)cdiv((long)h * w, LP_DPIX);
        pl->fin.off[l] = np;
        np += (long)B * pl->fin.chunks[l];
    }
    pl->n_partials = np;
    pl->buf_floats = (buf + 63) & ~(size_t)63;
    return true;
}

static inline size_t lp_ws_bytes(const LpPlan& pl) { return 2 * pl.buf_floats * sizeof(float) + (size_t)pl.n_partials * sizeof(double) + 256; }

}  // namespace evd

using namespace evd;

struct evd_lpips_model {
    DevBuf w[LP_L], b[LP_L], lin[LP_L];
    LpScale sc;
    void release() {
        for (int l = 0; l < LP_L; ++l) {
            w[l].release();
            b[l].release();
            lin[l].release();
        }
    }
};

extern "C" {

int evd_lpips_create(const evd_lpips_desc* d, evd_lpips_model** out) {
    EVD_REQUIRE(d && out, "evd_lpips_create: null argument");
    for (int l = 0; l < LP_L; ++l)
        EVD_REQUIRE(d->conv_w[l] && d->conv_b[l] && d->lin[l], "evd_lpips_create: layer %d: null weight, bias or head pointer", l);
    for (int c = 0; c < 3; ++c) EVD_REQUIRE(d->scale[c] != 0.f, "evd_lpips_create: scale[%d] is 0", c);
    evd_lpips_model* m = new evd_lpips_model();
    for (int c = 0; c < 3; ++c) {
        m->sc.shift[c] = d->shift[c];
        m->sc.scale[c] = d->scale[c];
    }
    for (int l = 0; l < LP_L; ++l) {
        // [Cout, Cin, kh, kw] -> [Kpad, Cout], k = (ky * ks + kx) * Cin + c; the rows past K are zero
        const int ks = LP_KS[l], ci = LP_CIN[l], co = LP_COUT[l], K = ks * ks * ci;
        const long kpad = cdiv(K, LP_KT) * LP_KT;
        std::vector<float> pk((size_t)kpad * co, 0.f);
        for (int o = 0; o < co; ++o)
            for (int c = 0; c < ci; ++c)
                for (int t = 0; t < ks * ks; ++t) pk[((size_t)t * ci + c) * co + o] = d->conv_w[l][((size_t)o * ci + c) * ks * ks + t];
        int rc = m->w[l].upload(pk.data(), pk.size() * sizeof(float));
        if (!rc) rc = m->b[l].upload(d->conv_b[l], sizeof(float) * co);
        if (!rc) rc = m->lin[l].upload(d->lin[l], sizeof(float) * co);
        if (rc) {
            m->release();
            delete m;
            return rc;
        }
    }
    *out = m;
    return EVD_OK;
}

void evd_lpips_destroy(evd_lpips_model* m) {
    if (!m) return;
    m->release();
    delete m;
}

size_t evd_lpips_workspace_bytes(int B, int H, int W) {
    LpPlan pl;
    return lp_plan(B, H, W, &pl) ? lp_ws_bytes(pl) : 0;
}

int evd_lpips(const evd_lpips_model* m, const float* pred, const float* target, int B, int H, int W, double* out, void* workspace, size_t workspace_bytes,
              void* stream) {
    EVD_REQUIRE(B >= 1, "evd_lpips: B=%d", B);
    EVD_REQUIRE(H >= EVD_LPIPS_MIN_SIDE && W >= EVD_LPIPS_MIN_SIDE,
                "evd_lpips: frames of %d x %d: each side must be at least %d (the second pool needs one output)", H, W, EVD_LPIPS_MIN_SIDE);
    LpPlan pl;
    EVD_REQUIRE(lp_plan(B, H, W, &pl), "evd_lpips: %d frames of %d x %d are too large", B, H, W);
    EVD_REQUIRE(m && pred && target && out, "evd_lpips: null argument");
    const size_t need = lp_ws_bytes(pl);
    EVD_REQUIRE(workspace && workspace_bytes >= need, "evd_lpips: workspace %zu < %zu bytes", workspace_bytes, need);
    hipStream_t st = as_stream(stream);
    float* buf[2];
    buf[0] = (float*)ws_align_ptr(workspace);
    buf[1] = buf[0] + pl.buf_floats;
    double* partials = (double*)(buf[1] + pl.buf_floats);

    const float* x = nullptr;            // the current layer's input
    int cur = 0;                         // the buffer the next stage writes
    for (int l = 0; l < LP_L; ++l) {
        const LpConv& c = pl.conv[l];
        if (LP_POOL[l]) {
            const LpConv& pc = pl.conv[l - 1];
            const long total4 = 2L * B * pl.pool_h[l] * pl.pool_w[l] * (c.Cin / 4);
            k_lpips_pool<<<(unsigned)cdiv(total4, 256L), 256, 0, st>>>(x, pc.Hout, pc.Wout, c.Cin, pl.pool_h[l], pl.pool_w[l], total4, buf[cur]);
            x = buf[cur];
            cur ^= 1;
        }
        const dim3 grid((unsigned)cdiv(c.M, LP_BM), (unsigned)(c.Cout / LP_BN));
        const float* w = (const float*)m->w[l].p;
        const float* bias = (const float*)m->b[l].p;
        if (l == 0)
            k_lpips_conv<true><<<grid, LP_THREADS, 0, st>>>(pred, target, B, w, bias, c, m->sc, buf[cur]);
        else
            k_lpips_conv<false><<<grid, LP_THREADS, 0, st>>>(x, nullptr, B, w, bias, c, m->sc, buf[cur]);
        x = buf[cur];
        cur ^= 1;
        k_lpips_dist<<<dim3((unsigned)pl.fin.chunks[l], (unsigned)B), 256, 0, st>>>(x, (const float*)m->lin[l].p, B, pl.fin.hw[l], c.Cout,
                                                                                   partials + pl.fin.off[l]);
    }
    k_lpips_finish<<<1, LP_FINISH_THREADS, 0, st>>>(partials, pl.fin, B, out);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

}  // extern "C"
