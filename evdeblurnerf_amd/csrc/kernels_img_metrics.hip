// Image metrics of the test-set pass on the device: compute_img_metric(rgbs, target, 'mse' | 'psnr' | 'ssim') (reference
// utils/metrics.py:18-100, called at run_nerf.py:685-687,704) in one main launch plus a fixed-order finish launch, and to8b
// (utils/misc.py:6).  The reference copies every frame to the host and runs three scikit-image passes in float32; here:
//   k_img_metrics         one workgroup per 16 x 32 tile of one image's region (the frame minus the margin, a window into the frames: no
//                         copy).  The tile and its halo of 3 are mapped, clamp(2 x - 1, -1, 1) in float32 (:48-49), into LDS for the three
//                         channels; everything after that is float64.  Per channel the five window moments (sum x, y, xx, yy, xy over
//                         7 x 7) come from separable sums: a horizontal pass over the 22 halo rows into LDS, a vertical pass per output
//                         pixel.  The halo is read with scipy.ndimage.uniform_filter's default border (half-sample symmetric `reflect`),
//                         which only the masked form looks at: without a mask the SSIM mean runs over the region shrunk by 3.
//                         The workgroup writes 5 partials: sum of squared differences, minimum of the (masked) prediction, sum of
//                         S x weight, sum of weight, sum of the mask's channel 0.
//   k_img_metrics_finish  one workgroup of 16 wavefronts; a wavefront per image sums that image's partials in a fixed order (lane l takes tiles l, l + 64,
//                         ..., then a butterfly), forms mse, psnr, ssim, and the three batch means are summed image by image.
// No floating-point atomics: two runs give the same bits, and an image's values do not depend on the rest of the batch (the grid is
// tiles x images; no sum crosses an image before the means).
// One deliberate deviation from the reference: each image is multiplied by ITS OWN mask.  The reference multiplies the whole batch by
// every earlier image's mask inside its loop (:77-78), which agrees with this for a batch of one or for identical binary masks.
// Thread mapping: 256 threads = 4 wavefronts; output pixel (row, col) of the tile belongs to thread (row / 2) * 32 + col, two neighbouring
// rows per thread (their vertical windows share 6 of 8 LDS rows), so a wavefront reads two full 32-wide rows of the LDS planes per access
// (stride 1: conflict-free).  LDS: 2 x 3 x 22 x 38 floats + 5 x 22 x 32
// doubles = 48 KB, three workgroups per CU.  The work is small (8 frames of 400 x 400: 31 MB read once, ~0.8 GFLOP of float64).
#include "evd_common.h"

namespace evd {

constexpr int IM_TH = EVD_IMG_METRICS_TILE_H, IM_TW = EVD_IMG_METRICS_TILE_W;
constexpr int IM_R = 3;                                  // the 7 x 7 window's radius
constexpr int IM_HH = IM_TH + 2 * IM_R, IM_HW = IM_TW + 2 * IM_R;
constexpr int IM_THREADS = 256;
constexpr int IM_FINISH_THREADS = 1024;                  // 16 wavefronts: 16 images at a time
constexpr int IM_NPART = 5;                              // sse, min, sum S w, sum w, sum mask[..., 0]
static_assert(IM_TW == 32 && IM_TH == 16 && IM_THREADS == 256, "thread mapping: 32 columns, two rows per thread");

// structural_similarity's constants with the reference's arguments: K1 0.01, K2 0.03, data_range 2 (float images), 7 x 7 sample covariance
constexpr double IM_C1 = (0.01 * 2.0) * (0.01 * 2.0), IM_C2 = (0.03 * 2.0) * (0.03 * 2.0);
constexpr double IM_INV_NP = 1.0 / 49.0, IM_COV_NORM = 49.0 / 48.0;     // (a window mean is sum x (1 / 49): one rounding more than a division, 1e-16 relative)

// (im * 2 - 1).clamp(-1, 1) in float32; NaN stays NaN
__device__ __forceinline__ float im_map(float v) {
    v = v * 2.f - 1.f;
    return v < -1.f ? -1.f : (v > 1.f ? 1.f : v);
}

// scipy.ndimage `reflect` (d c b a | a b c d | d c b a), branch-free; the last max only matters for halo pixels no output of the region uses
__device__ __forceinline__ int im_reflect(int i, int n) {
    i = max(i, -1 - i);
    return max(min(i, 2 * n - 1 - i), 0);
}

__device__ __forceinline__ double im_wave_sum(double v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double im_wave_min(double v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}

// pred, target [B, H, W, 3]; mask [B, H, W, mask_ch] or null; region rows r0 .. r0 + Hr, columns c0 .. c0 + Wr; blockIdx.x = image * tiles + tile
__global__ __launch_bounds__(IM_THREADS) void k_img_metrics(const float* __restrict__ pred, const float* __restrict__ target,
                                                            const float* __restrict__ mask, int mask_ch, int H, int W, int r0, int c0, int Hr, int Wr,
                                                            int tiles_x, int tiles, double* __restrict__ partials) {
    __shared__ float s_x[3][IM_HH][IM_HW], s_y[3][IM_HH][IM_HW];
    __shared__ double s_h[5][IM_HH][IM_TW];
    __shared__ double s_red[IM_THREADS / 64][IM_NPART];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / tiles, t = blockIdx.x - b * tiles;
    const int ty0 = (t / tiles_x) * IM_TH, tx0 = (t % tiles_x) * IM_TW;
    const long img = (long)b * H * W;                    // offsets inside an image fit 32 bits (H W 3 < 2^31, checked by the entry)
    const float* __restrict__ pimg = pred + img * 3;
    const float* __restrict__ timg = target + img * 3;
    const float* __restrict__ mimg = mask ? mask + img * mask_ch : nullptr;

    // Staging: a thread keeps one element (pixel, channel) of the 114-float halo row and walks down the rows, two rows per pass of the
    // workgroup, so the column's reflection and channel are computed once.  Every load is issued before the first value is used: one
    // exposed memory latency per workgroup, not IM_STAGE.
    constexpr int IM_STAGE = IM_HH / 2;
    static_assert(IM_HW * 3 <= IM_THREADS / 2 && IM_HH % 2 == 0, "staging: two halo rows per pass");
    const int e = tid & (IM_THREADS / 2 - 1), hr0 = tid / (IM_THREADS / 2);
    const bool stage = e < IM_HW * 3;
    const int hc = stage ? e / 3 : 0, sch = stage ? e % 3 : 0;
    const int gcol = (c0 + im_reflect(tx0 + hc - IM_R, Wr)) * 3 + sch;
    float vx[IM_STAGE], vy[IM_STAGE];
#pragma unroll
    for (int k = 0; k < IM_STAGE; ++k) {
        const int g = (r0 + im_reflect(ty0 + 2 * k + hr0 - IM_R, Hr)) * W * 3 + gcol;
        vx[k] = pimg[g];
        vy[k] = timg[g];
    }
    if (stage) {
#pragma unroll
        for (int k = 0; k < IM_STAGE; ++k) {
            s_x[sch][2 * k + hr0][hc] = im_map(vx[k]);
            s_y[sch][2 * k + hr0][hc] = im_map(vy[k]);
        }
    }
    __syncthreads();

    const int col = tid & 31, row0 = (tid >> 5) * 2;
    const int gc = tx0 + col;
    double sse = 0.0, mn = INFINITY, ssum = 0.0, wsum = 0.0, m0sum = 0.0;
    // mean_squared_error / the minimum peak_signal_noise_ratio looks at, on the (masked) centre pixels
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int row = row0 + k, gr = ty0 + row;
        if (gr < Hr && gc < Wr) {
            const float* mp = mimg ? mimg + ((r0 + gr) * W + (c0 + gc)) * mask_ch : nullptr;
            if (mp) m0sum += (double)mp[0];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                double x = (double)s_x[ch][row + IM_R][col + IM_R], y = (double)s_y[ch][row + IM_R][col + IM_R];
                if (mp) {
                    const double m = (double)mp[mask_ch == 3 ? ch : 0];
                    x *= m;
                    y *= m;
                }
                const double d = x - y;
                sse += d * d;
                mn = fmin(mn, x);
            }
        }
    }

    for (int ch = 0; ch < 3; ++ch) {
        for (int i = tid; i < IM_HH * IM_TW; i += IM_THREADS) {
            const int hr = i >> 5, c = i & 31;
            double ax = 0.0, ay = 0.0, axx = 0.0, ayy = 0.0, axy = 0.0;
#pragma unroll
            for (int j = 0; j < 2 * IM_R + 1; ++j) {
                const double x = (double)s_x[ch][hr][c + j], y = (double)s_y[ch][hr][c + j];
                ax += x;
                ay += y;
                axx += x * x;
                ayy += y * y;
                axy += x * y;
            }
            s_h[0][hr][c] = ax;
            s_h[1][hr][c] = ay;
            s_h[2][hr][c] = axx;
            s_h[3][hr][c] = ayy;
            s_h[4][hr][c] = axy;
        }
        __syncthreads();
        double a[2][5];                                  // the window means of the thread's two rows: 8 LDS rows, 6 of them shared
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            double r[2 * IM_R + 2];
#pragma unroll
            for (int j = 0; j < 2 * IM_R + 2; ++j) r[j] = s_h[m][row0 + j][col];
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int j = 0; j < 2 * IM_R + 1; ++j) {
                s0 += r[j];
                s1 += r[j + 1];
            }
            a[0][m] = s0 * IM_INV_NP;
            a[1][m] = s1 * IM_INV_NP;
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int gr = ty0 + row0 + k;
            if (gr < Hr && gc < Wr) {
                const double ux = a[k][0], uy = a[k][1];
                const double vx = IM_COV_NORM * (a[k][2] - ux * ux), vy = IM_COV_NORM * (a[k][3] - uy * uy), vxy = IM_COV_NORM * (a[k][4] - ux * uy);
                const double A1 = 2.0 * ux * uy + IM_C1, A2 = 2.0 * vxy + IM_C2, B1 = ux * ux + uy * uy + IM_C1, B2 = vx + vy + IM_C2;
                const double S = (A1 * A2) / (B1 * B2);
                if (mimg) {                              // (ssimmap * mask[i]).sum() / mask[i].sum(), :91
                    const double m = (double)mimg[((r0 + gr) * W + (c0 + gc)) * mask_ch + (mask_ch == 3 ? ch : 0)];
                    ssum += S * m;
                    wsum += m;
                } else if (gr >= IM_R && gr < Hr - IM_R && gc >= IM_R && gc < Wr - IM_R) {      // crop(S, 3).mean()
                    ssum += S;
                    wsum += 1.0;
                }
            }
        }
        __syncthreads();
    }

    const int wave = tid >> 6, lane = tid & 63;
    sse = im_wave_sum(sse);
    mn = im_wave_min(mn);
    ssum = im_wave_sum(ssum);
    wsum = im_wave_sum(wsum);
    m0sum = im_wave_sum(m0sum);
    if (lane == 0) {
        s_red[wave][0] = sse;
        s_red[wave][1] = mn;
        s_red[wave][2] = ssum;
        s_red[wave][3] = wsum;
        s_red[wave][4] = m0sum;
    }
    __syncthreads();
    if (tid < IM_NPART) {
        double v = s_red[0][tid];
        for (int w = 1; w < IM_THREADS / 64; ++w) v = tid == 1 ? fmin(v, s_red[w][tid]) : v + s_red[w][tid];
        partials[(long)blockIdx.x * IM_NPART + tid] = v;
    }
}

// out: mse [B], psnr [B], ssim [B], mean mse, mean psnr, mean ssim
__global__ __launch_bounds__(IM_FINISH_THREADS) void k_img_metrics_finish(const double* __restrict__ partials, int B, int tiles, int Hr, int Wr, int has_mask,
                                                                   double* __restrict__ out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int b = wave; b < B; b += IM_FINISH_THREADS / 64) {
        const double* p = partials + (long)b * tiles * IM_NPART;
        double sse = 0.0, mn = INFINITY, ssum = 0.0, wsum = 0.0, m0sum = 0.0;
        for (int t = lane; t < tiles; t += 64) {
            sse += p[t * IM_NPART];
            mn = fmin(mn, p[t * IM_NPART + 1]);
            ssum += p[t * IM_NPART + 2];
            wsum += p[t * IM_NPART + 3];
            m0sum += p[t * IM_NPART + 4];
        }
        sse = im_wave_sum(sse);
        mn = im_wave_min(mn);
        ssum = im_wave_sum(ssum);
        wsum = im_wave_sum(wsum);
        m0sum = im_wave_sum(m0sum);
        if (lane == 0) {
            double mse = sse / ((double)Hr * (double)Wr * 3.0);
            const double range = mn >= 0.0 ? 1.0 : 2.0;  // peak_signal_noise_ratio: dmax if the first image has no negative value, else dmax - dmin
            double psnr = 10.0 * log10(range * range / mse);
            if (has_mask) {                              // value - 10 log10(h w / mask[i, ..., 0].sum()), for both (:83-85)
                const double corr = 10.0 * log10((double)Hr * (double)Wr / m0sum);
                mse -= corr;
                psnr -= corr;
            }
            out[b] = mse;
            out[B + b] = psnr;
            out[2 * (long)B + b] = ssum / wsum;
        }
    }
    __syncthreads();
    if (threadIdx.x < 3) {                               // sum(values) / len(values), image by image (:100)
        const double* v = out + (long)threadIdx.x * B;
        double s = 0.0;
        for (int b = 0; b < B; ++b) s += v[b];
        out[3 * (long)B + threadIdx.x] = s / (double)B;
    }
}

// 4 values per thread; `vec`: x 16-byte and out 4-byte aligned (the last n % 4 values go one by one)
__global__ __launch_bounds__(256) void k_to8b(const float* __restrict__ x, long n, unsigned char* __restrict__ out, int vec) {
    const long i = (blockIdx.x * 256L + threadIdx.x) * 4;
    if (i >= n) return;
    if (vec && i + 4 <= n) {
        const float4 v = *reinterpret_cast<const float4*>(x + i);
        uchar4 o;
        o.x = to8b_u8(v.x);
        o.y = to8b_u8(v.y);
        o.z = to8b_u8(v.z);
        o.w = to8b_u8(v.w);
        *reinterpret_cast<uchar4*>(out + i) = o;
    } else {
        for (long j = i; j < n && j < i + 4; ++j) out[j] = to8b_u8(x[j]);
    }
}

static inline long im_tiles(int h, int w) { return cdiv(h, IM_TH) * cdiv(w, IM_TW); }
static inline size_t im_ws_bytes(int B, int h, int w) { return (size_t)B * im_tiles(h, w) * IM_NPART * sizeof(double) + 256; }

}  // namespace evd

using namespace evd;

extern "C" {

size_t evd_img_metrics_workspace_bytes(int B, int H, int W) {
    if (B < 1 || H < 2 * IM_R + 1 || W < 2 * IM_R + 1 || (long)B * im_tiles(H, W) >= (1L << 31)) return 0;
    return im_ws_bytes(B, H, W);
}

int evd_img_metrics(const float* pred, const float* target, const float* mask, int mask_ch, int B, int H, int W, int margin_h, int margin_w,
                    double* out, void* workspace, size_t workspace_bytes, void* stream) {
    EVD_REQUIRE(B >= 1 && H >= 1 && W >= 1 && (long)H * W * 3 < (1L << 31) && margin_h >= 0 && margin_w >= 0 && margin_h <= H / 2 && margin_w <= W / 2,
                "evd_img_metrics: bad sizes B=%d H=%d W=%d margin_h=%d margin_w=%d", B, H, W, margin_h, margin_w);
    const int Hr = H - 2 * margin_h, Wr = W - 2 * margin_w;
    EVD_REQUIRE(Hr >= 2 * IM_R + 1 && Wr >= 2 * IM_R + 1, "evd_img_metrics: the region %d x %d (frame %d x %d, margins %d, %d) is smaller than the 7 x 7 window",
                Hr, Wr, H, W, margin_h, margin_w);
    EVD_REQUIRE(!mask || mask_ch == 1 || mask_ch == 3, "evd_img_metrics: mask_ch %d (1 or 3)", mask_ch);
    const long tiles = im_tiles(Hr, Wr);
    EVD_REQUIRE((long)B * tiles < (1L << 31), "evd_img_metrics: %d images of %ld tiles: too many workgroups", B, tiles);
    EVD_REQUIRE(pred && target && out, "evd_img_metrics: null argument");
    const size_t need = im_ws_bytes(B, Hr, Wr);
    EVD_REQUIRE(workspace && workspace_bytes >= need, "evd_img_metrics: workspace %zu < %zu bytes", workspace_bytes, need);
    hipStream_t st = as_stream(stream);
    double* partials = (double*)ws_align_ptr(workspace);
    k_img_metrics<<<(unsigned)(B * tiles), IM_THREADS, 0, st>>>(pred, target, mask, mask_ch, H, W, margin_h, margin_w, Hr, Wr, (int)cdiv(Wr, IM_TW), (int)tiles,
                                                                partials);
    k_img_metrics_finish<<<1, IM_FINISH_THREADS, 0, st>>>(partials, B, (int)tiles, Hr, Wr, mask ? 1 : 0, out);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int evd_to8b(const float* x, long n, unsigned char* out, void* stream) {
    EVD_REQUIRE(n >= 0 && n < (1L << 40), "evd_to8b: bad size n=%ld", n);
    if (n == 0) return EVD_OK;
    EVD_REQUIRE(x && out, "evd_to8b: null argument");
    const int vec = ((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 3) == 0;
    k_to8b<<<(unsigned)cdiv(cdiv(n, 4L), 256L), 256, 0, as_stream(stream)>>>(x, n, out, vec);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

}  // extern "C"
