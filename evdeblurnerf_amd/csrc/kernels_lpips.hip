// LPIPS of the test-set pass on the device: compute_img_metric(rgbs, target, 'lpips') (reference utils/metrics.py:92-95, called at
// run_nerf.py:688), i.e. networks/lpips/lpips.py LPIPS in eval mode: a convolutional backbone on both frames -- the first five convolutions
// of AlexNet (net='alex') or VGG-16 features[0:30] (net='vgg'), one layer table each (LP_NETS) -- and per tapped layer the head-weighted
// squared distance of the channel-normalised features, averaged over the pixels (evd_lpips) or upsampled to the frame and added per pixel
// (spatial=True, evd_lpips_spatial).  The baseline without heads (lpips=False) is heads of exact ones; version 0.0 is shift 0, scale 1.  The
// reference copies every frame to the host and runs the convolutions on the CPU; here everything stays on the caller's stream.  The
// weights are the caller's (evd_lpips_create, evd_lpips_create_net); float32 features, float64 from the normalisation on.
//   k_lpips_conv<FIRST>   implicit GEMM on v_mfma_f32_32x32x2_f32 (exact float32 products) over channel-last activations [2 B, h, w, C]: the
//                         predicted and the target frames of the whole batch in one launch, M = 2 B ho wo rows (one per output pixel),
//                         N = Cout, K = (ky, kx, c) with c fastest, so that a K tile of 32 is 128 contiguous bytes of one tap.  Weights are
//                         packed once to [Kpad, Cout].  A workgroup of 4 wavefronts owns a 128 x 64 tile, a wavefront 32 rows x 64 columns
//                         (two accumulators: one A read feeds two MFMAs).  Zero padding and the M edge are predicates on the A load.  The
//                         next K tile's global loads are issued before the current tile's MFMAs.  A K tile is summed from zero and then
//                         added to the running accumulator (blocked summation: the chain a rounding error travels through is
//                         16 + K / 32 additions, not K / 2).  Epilogue: + bias, ReLU.  FKS > 0 (the first convolution, Cin 3, FKS x FKS:
//                         AlexNet's K 363, VGG's K 27 in one K tile): reads the caller's [B, H, W, 3] frames, pred then target, and applies
//                         clamp(2 x - 1, -1, 1) (utils/metrics.py:48-49) and the scaling layer (x - shift) / scale (lpips.py:245-252) on
//                         load, element by element.
//   k_lpips_pool<WIN, STR> MaxPool(WIN, stride STR, floor), channel-last, float4: (3, 2) in front of AlexNet's conv2 and conv3, (2, 2) in
//                         front of VGG's conv2_1, 3_1, 4_1 and 5_1.
//   k_lpips_dist<MAP>     per tapped layer: a wavefront per pixel, n = sqrt(sum_c f^2) for both frames and
//                         d = sum_c lin_c (f0_c / (n0 + 1e-10) - f1_c / (n1 + 1e-10))^2 in float64 by butterflies; a workgroup sums its 64
//                         pixels in a fixed order into one float64 partial, or (MAP) stores every pixel's d to the layer's float64 map.
//   k_lpips_finish        one workgroup: a wavefront per (image, layer) sums that pair's partials in a fixed order and divides by the pixel
//                         count; the five terms are added layer by layer, the batch mean image by image.
//   k_lpips_upsample      spatial: a thread per output pixel reads the five maps bilinearly (nn.Upsample(size=(H, W), mode='bilinear',
//                         align_corners=False), lpips.py:134-136), adds them in layer order in float64 and rounds once to float32.
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

constexpr int LP_MAXC = EVD_LPIPS_MAX_CONVS;

// One convolution of a backbone: Cin -> Cout, kernel / stride / pad, the floor-mode max pool in front of it, and whether its output
// (after the ReLU) is one of the five taps the distance is taken at
enum { LP_POOL_NONE = 0, LP_POOL_3_2 = 1, LP_POOL_2_2 = 2 };
struct LpLayer {
    int cin, cout, ks, stride, pad, pool;
    bool tap;
};
struct LpNet {
    const char* name;
    int n, min_side;                     // convolutions; the smallest side at which the last pool still has one output
    LpLayer layer[LP_MAXC];
};
constexpr int lp_pool_win(int pool) { return pool == LP_POOL_3_2 ? 3 : 2; }
constexpr LpNet LP_NETS[2] = {
    // AlexNet features[0:12] (torchvision): every convolution is a tap
    {"alex", 5, EVD_LPIPS_MIN_SIDE,
     {{3, 64, 11, 4, 2, LP_POOL_NONE, true}, {64, 192, 5, 1, 2, LP_POOL_3_2, true}, {192, 384, 3, 1, 1, LP_POOL_3_2, true},
      {384, 256, 3, 1, 1, LP_POOL_NONE, true}, {256, 256, 3, 1, 1, LP_POOL_NONE, true}}},
    // VGG-16 features[0:30] (torchvision): taps at relu1_2, 2_2, 3_3, 4_3, 5_3 (pretrained_networks.py:98-136)
    {"vgg16", 13, EVD_LPIPS_VGG_MIN_SIDE,
     {{3, 64, 3, 1, 1, LP_POOL_NONE, false}, {64, 64, 3, 1, 1, LP_POOL_NONE, true},
      {64, 128, 3, 1, 1, LP_POOL_2_2, false}, {128, 128, 3, 1, 1, LP_POOL_NONE, true},
      {128, 256, 3, 1, 1, LP_POOL_2_2, false}, {256, 256, 3, 1, 1, LP_POOL_NONE, false}, {256, 256, 3, 1, 1, LP_POOL_NONE, true},
      {256, 512, 3, 1, 1, LP_POOL_2_2, false}, {512, 512, 3, 1, 1, LP_POOL_NONE, false}, {512, 512, 3, 1, 1, LP_POOL_NONE, true},
      {512, 512, 3, 1, 1, LP_POOL_2_2, false}, {512, 512, 3, 1, 1, LP_POOL_NONE, false}, {512, 512, 3, 1, 1, LP_POOL_NONE, true}}}};
static_assert(EVD_LPIPS_NET_ALEX == 0 && EVD_LPIPS_NET_VGG16 == 1, "LP_NETS is indexed by the backbone id");

struct LpConv {
    int Hin, Win, Cin, Hout, Wout, Cout, ks, stride, pad, K, nkt;
    int M;                               // 2 B Hout Wout
};
struct LpScale {
    float shift[3], scale[3];
};
struct LpFinish {                        // per tap
    long off[LP_L];                      // the layer's first partial
    int chunks[LP_L];                    // partials per image
    int hw[LP_L];                        // pixels per image
};
struct LpMaps {                          // per tap: the float64 distance maps [B, h, w] of the spatial entry
    long off[LP_L];
    int h[LP_L], w[LP_L];
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
// FKS: 0, or the kernel size of a first convolution (FIRST), a compile-time constant so that the per-element decode divides by constants
template <int FKS>
__global__ __launch_bounds__(LP_THREADS) void k_lpips_conv(const float* __restrict__ in, const float* __restrict__ in2, int B,
                                                          const float* __restrict__ wpk, const float* __restrict__ bias, LpConv g, LpScale sc,
                                                          float* __restrict__ out) {
    __shared__ float s_a[LP_BM][LP_ALD];
    __shared__ float s_b[LP_KT][LP_BLD];
    constexpr bool FIRST = FKS > 0;
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
        if constexpr (FIRST) {           // Cin 3: k = (ky * FKS + kx) * 3 + c, decoded per element; k >= K reads as 0
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int k = k0 + akq + j;
                const int ky = k / (3 * FKS), r = k - ky * (3 * FKS), kx = r / 3, c = r - kx * 3;
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

// MaxPool2d(WIN, stride STR), floor: every window lies inside the map.  x [N, Hin, Win, C] -> y [N, Ho, Wo, C], C a multiple of 4; NaN wins
template <int WIN, int STR>
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
    const float4* src = reinterpret_cast<const float4*>(x) + ((n * Hin + STR * oy) * Win + STR * ox) * c4 + c;
    float4 m = src[0];
#pragma unroll
    for (int dy = 0; dy < WIN; ++dy)
#pragma unroll
        for (int dx = 0; dx < WIN; ++dx) {
            const float4 v = src[((long)dy * Win + dx) * c4];
            m.x = (v.x > m.x || v.x != v.x) ? v.x : m.x;
            m.y = (v.y > m.y || v.y != v.y) ? v.y : m.y;
            m.z = (v.z > m.z || v.z != v.z) ? v.z : m.z;
            m.w = (v.w > m.w || v.w != v.w) ? v.w : m.w;
        }
    reinterpret_cast<float4*>(y)[i] = m;
}

// feat [2 B, hw, C]: image b's predicted frame is row block b, its target row block B + b.  grid (chunks, B); out: partials [B, chunks],
// or (MAP) the per-pixel distances [B, hw]
template <bool MAP>
__global__ __launch_bounds__(256) void k_lpips_dist(const float* __restrict__ feat, const float* __restrict__ lin, int B, int hw, int C,
                                                    double* __restrict__ out) {
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
        d = lp_wave_sum(d);
        if constexpr (MAP) {
            if (lane == 0) out[(long)b * hw + p] = d;
        } else {
            acc += d;
        }
    }
    if constexpr (!MAP) {
        if (lane == 0) s_red[wave] = acc;
        __syncthreads();
        if (threadIdx.x == 0) out[(long)b * gridDim.x + blockIdx.x] = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
    }
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

// maps: the five float64 distance maps (LpMaps); out [B, H, W]; layers [B, 5, H, W] or null.  nn.Upsample(size=(H, W), mode='bilinear',
// align_corners=False) per layer: source coordinate (dst + 0.5) in / out - 0.5, clamped below at 0, the upper neighbour clamped to the last
// index; the five are added in layer order (val = res[0]; val += res[l]) in float64 and rounded once
__device__ __forceinline__ void lp_src(int dst, int in, int out, int* i0, int* i1, double* l1) {
    double s = ((double)in / (double)out) * ((double)dst + 0.5) - 0.5;
    s = s < 0.0 ? 0.0 : s;
    int i = (int)s;
    i = i > in - 1 ? in - 1 : i;
    *i0 = i;
    *i1 = i + (i < in - 1 ? 1 : 0);
    *l1 = s - (double)i;
}

__global__ __launch_bounds__(256) void k_lpips_upsample(const double* __restrict__ maps, LpMaps f, int B, int H, int W, float* __restrict__ out,
                                                        float* __restrict__ layers) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= (long)B * H * W) return;
    const int x = (int)(i % W);
    const long q = i / W;
    const int y = (int)(q % H);
    const long b = q / H;
    double v = 0.0;
#pragma unroll
    for (int l = 0; l < LP_L; ++l) {
        int y0, y1, x0, x1;
        double ly, lx;
        lp_src(y, f.h[l], H, &y0, &y1, &ly);
        lp_src(x, f.w[l], W, &x0, &x1, &lx);
        const double* m = maps + f.off[l] + b * f.h[l] * f.w[l];
        const double r0 = (1.0 - lx) * m[(long)y0 * f.w[l] + x0] + lx * m[(long)y0 * f.w[l] + x1];
        const double r1 = (1.0 - lx) * m[(long)y1 * f.w[l] + x0] + lx * m[(long)y1 * f.w[l] + x1];
        const double u = (1.0 - ly) * r0 + ly * r1;
        if (layers) layers[((b * LP_L + l) * H + y) * W + x] = (float)u;
        v = l == 0 ? u : v + u;
    }
    out[i] = (float)v;
}

// sizes of every stage for B frames of H x W
struct LpPlan {
    LpConv conv[LP_MAXC];
    int pool_h[LP_MAXC], pool_w[LP_MAXC]; // the pooled map in front of a convolution (0: no pool)
    int tap[LP_MAXC];                    // the convolution's tap index, or -1
    LpFinish fin;
    LpMaps maps;
    long n_partials, n_map;
    size_t buf_floats;                   // each of the two activation buffers
};

static bool lp_plan(const LpNet& net, int B, int H, int W, LpPlan* pl) {
    if (B < 1 || H < net.min_side || W < net.min_side || (long)H * W * 3 >= (1L << 31)) return false;
    int h = H, w = W, t = 0;
    long np = 0, nm = 0;
    size_t buf = 0;
    for (int l = 0; l < net.n; ++l) {
        const LpLayer& ly = net.layer[l];
        if (ly.pool != LP_POOL_NONE) {
            const int win = lp_pool_win(ly.pool);
            h = (h - win) / 2 + 1;
            w = (w - win) / 2 + 1;
            pl->pool_h[l] = h;
            pl->pool_w[l] = w;
            buf = std::max(buf, (size_t)2 * B * h * w * ly.cin);
        } else {
            pl->pool_h[l] = pl->pool_w[l] = 0;
        }
        LpConv& c = pl->conv[l];
        c.Hin = h;
        c.Win = w;
        c.Cin = ly.cin;
        c.ks = ly.ks;
        c.stride = ly.stride;
        c.pad = ly.pad;
        c.Cout = ly.cout;
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
        pl->tap[l] = ly.tap ? t : -1;
        if (ly.tap) {
            pl->fin.hw[t] = h * w;
            pl->fin.chunks[t] = (int)cdiv((long)h * w, LP_DPIX);
            pl->fin.off[t] = np;
            np += (long)B * pl->fin.chunks[t];
            pl->maps.h[t] = h;
            pl->maps.w[t] = w;
            pl->maps.off[t] = nm;
            nm += (long)B * h * w;
            ++t;
        }
    }
    pl->n_partials = np;
    pl->n_map = nm;
    pl->buf_floats = (buf + 63) & ~(size_t)63;
    return true;
}

// two activation buffers, then the float64 partials (evd_lpips) or the five float64 maps (evd_lpips_spatial)
static inline size_t lp_ws_bytes(const LpPlan& pl, bool spatial) {
    return 2 * pl.buf_floats * sizeof(float) + (size_t)(spatial ? pl.n_map : pl.n_partials) * sizeof(double) + 256;
}

}  // namespace evd

using namespace evd;

struct evd_lpips_model {
    int net;                             // EVD_LPIPS_NET_*: first, the one member an entry reads before it has validated the sizes
    DevBuf w[LP_MAXC], b[LP_MAXC], lin[LP_L];
    LpScale sc;
    void release() {
        for (int l = 0; l < LP_MAXC; ++l) {
            w[l].release();
            b[l].release();
        }
        for (int l = 0; l < LP_L; ++l) lin[l].release();
    }
};

static inline bool lp_net_ok(int net) { return net == EVD_LPIPS_NET_ALEX || net == EVD_LPIPS_NET_VGG16; }

// the backbone and the per-tap distance kernel (partials or maps) on `st`: the launches of both entries
template <bool MAP>
static void lp_run(const evd_lpips_model* m, const LpNet& net, const LpPlan& pl, const float* pred, const float* target, int B, float* const buf[2],
                   double* dist, hipStream_t st) {
    const float* x = nullptr;            // the current layer's input
    int cur = 0;                         // the buffer the next stage writes
    for (int l = 0; l < net.n; ++l) {
        const LpConv& c = pl.conv[l];
        if (net.layer[l].pool != LP_POOL_NONE) {
            const LpConv& pc = pl.conv[l - 1];
            const long total4 = 2L * B * pl.pool_h[l] * pl.pool_w[l] * (c.Cin / 4);
            const unsigned blocks = (unsigned)cdiv(total4, 256L);
            if (net.layer[l].pool == LP_POOL_3_2)
                k_lpips_pool<3, 2><<<blocks, 256, 0, st>>>(x, pc.Hout, pc.Wout, c.Cin, pl.pool_h[l], pl.pool_w[l], total4, buf[cur]);
            else
                k_lpips_pool<2, 2><<<blocks, 256, 0, st>>>(x, pc.Hout, pc.Wout, c.Cin, pl.pool_h[l], pl.pool_w[l], total4, buf[cur]);
            x = buf[cur];
            cur ^= 1;
        }
        const dim3 grid((unsigned)cdiv(c.M, LP_BM), (unsigned)(c.Cout / LP_BN));
        const float* w = (const float*)m->w[l].p;
        const float* bias = (const float*)m->b[l].p;
        if (l == 0 && c.ks == 11)
            k_lpips_conv<11><<<grid, LP_THREADS, 0, st>>>(pred, target, B, w, bias, c, m->sc, buf[cur]);
        else if (l == 0)
            k_lpips_conv<3><<<grid, LP_THREADS, 0, st>>>(pred, target, B, w, bias, c, m->sc, buf[cur]);
        else
            k_lpips_conv<0><<<grid, LP_THREADS, 0, st>>>(x, nullptr, B, w, bias, c, m->sc, buf[cur]);
        x = buf[cur];
        cur ^= 1;
        const int t = pl.tap[l];
        if (t < 0) continue;             // not a tap: only the next convolution's input
        double* o = dist + (MAP ? pl.maps.off[t] : pl.fin.off[t]);
        k_lpips_dist<MAP><<<dim3((unsigned)pl.fin.chunks[t], (unsigned)B), 256, 0, st>>>(x, (const float*)m->lin[t].p, B, pl.fin.hw[t], c.Cout, o);
    }
}

// the checks both entries share, in the order every entry keeps (nothing of the device, and of the handle only its backbone id, is read
// before the sizes are validated), and the carve of the workspace
struct LpCall {
    const LpNet* net;
    LpPlan pl;
    float* buf[2];
    double* dist;                        // the partials (evd_lpips) or the maps (evd_lpips_spatial)
};

static int lp_prepare(const char* entry, const evd_lpips_model* m, const void* pred, const void* target, const void* out, int B, int H, int W,
                      void* workspace, size_t workspace_bytes, bool spatial, LpCall* c) {
    EVD_REQUIRE(B >= 1, "%s: B=%d", entry, B);
    EVD_REQUIRE(m && pred && target && out, "%s: null argument", entry);
    EVD_REQUIRE(lp_net_ok(m->net), "%s: the handle holds no known backbone (%d)", entry, m->net);
    const LpNet& net = LP_NETS[m->net];
    EVD_REQUIRE(H >= net.min_side && W >= net.min_side, "%s: %s: frames of %d x %d: each side must be at least %d (the last pool needs one output)",
                entry, net.name, H, W, net.min_side);
    EVD_REQUIRE(lp_plan(net, B, H, W, &c->pl), "%s: %s: %d frames of %d x %d are too large (a layer of 2 B h w >= 2^31 rows)", entry, net.name, B, H, W);
    const size_t need = lp_ws_bytes(c->pl, spatial);
    EVD_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace %zu < %zu bytes", entry, workspace_bytes, need);
    c->net = &net;
    c->buf[0] = (float*)ws_align_ptr(workspace);
    c->buf[1] = c->buf[0] + c->pl.buf_floats;
    c->dist = (double*)(c->buf[1] + c->pl.buf_floats);
    return EVD_OK;
}

static int lp_create(int netid, bool heads, const float* const* conv_w, const float* const* conv_b, const float* const* lin, const float* shift,
                     const float* scale, const char* entry, evd_lpips_model** out) {
    const LpNet& net = LP_NETS[netid];
    for (int l = 0; l < net.n; ++l)
        EVD_REQUIRE(conv_w[l] && conv_b[l], "%s: %s: convolution %d: null weight or bias pointer", entry, net.name, l);
    for (int t = 0; heads && t < LP_L; ++t) EVD_REQUIRE(lin[t], "%s: %s: heads requested, head %d is null", entry, net.name, t);
    for (int c = 0; c < 3; ++c) EVD_REQUIRE(scale[c] != 0.f, "%s: scale[%d] is 0", entry, c);
    evd_lpips_model* m = new evd_lpips_model();
    m->net = netid;
    for (int c = 0; c < 3; ++c) {
        m->sc.shift[c] = shift[c];
        m->sc.scale[c] = scale[c];
    }
    int t = 0;
    for (int l = 0; l < net.n; ++l) {
        // [Cout, Cin, kh, kw] -> [Kpad, Cout], k = (ky * ks + kx) * Cin + c; the rows past K are zero
        const int ks = net.layer[l].ks, ci = net.layer[l].cin, co = net.layer[l].cout, K = ks * ks * ci;
        const long kpad = cdiv(K, LP_KT) * LP_KT;
        std::vector<float> pk((size_t)kpad * co, 0.f);
        for (int o = 0; o < co; ++o)
            for (int c = 0; c < ci; ++c)
                for (int q = 0; q < ks * ks; ++q) pk[((size_t)q * ci + c) * co + o] = conv_w[l][((size_t)o * ci + c) * ks * ks + q];
        int rc = m->w[l].upload(pk.data(), pk.size() * sizeof(float));
        if (!rc) rc = m->b[l].upload(conv_b[l], sizeof(float) * co);
        if (!rc && net.layer[l].tap) {   // the baseline (lpips=False) is the plain channel sum: heads of exact ones, a product with 1.0 is exact
            const std::vector<float> ones((size_t)co, 1.f);
            rc = m->lin[t].upload(heads ? lin[t] : ones.data(), sizeof(float) * co);
            ++t;
        }
        if (rc) {
            m->release();
            delete m;
            return rc;
        }
    }
    *out = m;
    return EVD_OK;
}

extern "C" {

int evd_lpips_create(const evd_lpips_desc* d, evd_lpips_model** out) {
    EVD_REQUIRE(d && out, "evd_lpips_create: null argument");
    return lp_create(EVD_LPIPS_NET_ALEX, true, d->conv_w, d->conv_b, d->lin, d->shift, d->scale, "evd_lpips_create", out);
}

int evd_lpips_create_net(const evd_lpips_net_desc* d, evd_lpips_model** out) {
    EVD_REQUIRE(d && out, "evd_lpips_create_net: null argument");
    EVD_REQUIRE(lp_net_ok(d->net), "evd_lpips_create_net: unknown backbone %d (EVD_LPIPS_NET_ALEX = %d, EVD_LPIPS_NET_VGG16 = %d)", d->net,
                EVD_LPIPS_NET_ALEX, EVD_LPIPS_NET_VGG16);
    return lp_create(d->net, d->heads != 0, d->conv_w, d->conv_b, d->lin, d->shift, d->scale, "evd_lpips_create_net", out);
}

void evd_lpips_destroy(evd_lpips_model* m) {
    if (!m) return;
    m->release();
    delete m;
}

int evd_lpips_min_side(int net) { return lp_net_ok(net) ? LP_NETS[net].min_side : 0; }

size_t evd_lpips_workspace_bytes(int B, int H, int W) {
    LpPlan pl;
    return lp_plan(LP_NETS[EVD_LPIPS_NET_ALEX], B, H, W, &pl) ? lp_ws_bytes(pl, false) : 0;
}

size_t evd_lpips_model_workspace_bytes(const evd_lpips_model* m, int B, int H, int W, int spatial) {
    LpPlan pl;
    if (!m || !lp_net_ok(m->net)) return 0;
    return lp_plan(LP_NETS[m->net], B, H, W, &pl) ? lp_ws_bytes(pl, spatial != 0) : 0;
}

int evd_lpips(const evd_lpips_model* m, const float* pred, const float* target, int B, int H, int W, double* out, void* workspace, size_t workspace_bytes,
              void* stream) {
    LpCall c;
    if (int rc = lp_prepare("evd_lpips", m, pred, target, out, B, H, W, workspace, workspace_bytes, false, &c)) return rc;
    hipStream_t st = as_stream(stream);
    lp_run<false>(m, *c.net, c.pl, pred, target, B, c.buf, c.dist, st);
    k_lpips_finish<<<1, LP_FINISH_THREADS, 0, st>>>(c.dist, c.pl.fin, B, out);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int evd_lpips_spatial(const evd_lpips_model* m, const float* pred, const float* target, int B, int H, int W, float* map, float* layer_maps,
                      void* workspace, size_t workspace_bytes, void* stream) {
    LpCall c;
    if (int rc = lp_prepare("evd_lpips_spatial", m, pred, target, map, B, H, W, workspace, workspace_bytes, true, &c)) return rc;
    hipStream_t st = as_stream(stream);
    lp_run<true>(m, *c.net, c.pl, pred, target, B, c.buf, c.dist, st);
    k_lpips_upsample<<<(unsigned)cdiv((long)B * H * W, 256L), 256, 0, st>>>(c.dist, c.pl.maps, B, H, W, map, layer_maps);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

}  // extern "C"
