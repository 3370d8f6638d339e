// The EDI prior table on the device: LLFFEventsDataset.compute_edi_prior (reference data/loader_events.py:99-131) -- per blurry image
// `steps` boundary timestamps, the event window between each pair of neighbours, brightness_increment_image of every window
// (utils/edi.py:7-70, bilinear splat) and deblur_double_integral (:73-95) -- in three kernels on the resident event tables:
//   k_edi_windows       lower / upper bound of every boundary in the timestamp column (torch.searchsorted left / right, :111-112)
//   k_edi_prior_splat   one launch for every image of a chunk and every window: an event finds its window(s) by INDEX comparison
//                       (left[i, j] <= e < right[i, j + 1], :119-121 -- an event on an interior boundary is in two windows) and adds its
//                       bilinear taps into 64-bit integer planes (positive / negative polarity) with integer atomics
//   k_edi_prior_deblur  per pixel: bii_j = float(pos_j) c_pos - float(neg_j) c_neg (:69), the partial sums in the reference's order, expf,
//                       sharp = steps blurry / sum exp for the three channels
// Fixed point: one unit is EDI_Q = 2^-40.  A tap weight (1 - |xf - x|)(1 - |yf - y|) <= 1 is <= 2^40 units, so a pixel takes 2^23 unit taps per
// window and polarity before a signed 64-bit sum overflows.  The coordinates are float32 values held as float64 (EventTables keeps the
// float32 event coordinates): for coordinates >= 1 each factor has at most 23 significant bits and the float64 product is exact; it is
// then rounded to the nearest unit, so a stored weight is exact (coordinates >= 256: multiples of 2^-30) or off by at most 2^-41.  Integer
// sums do not depend on the arrival order: the table is bit-reproducible, unlike the float atomics of k_edi_splat below.
// One deviation from the reference: a tap with xf < 0 or yf < 0 is dropped (numpy wraps the negative index to the opposite edge).
// Thread-to-event mapping: one thread per event, consecutive threads on consecutive events of one image (blockIdx.y), a grid-stride loop over
// the image's index range, so that no size has to be read back.  The four taps of an event are two 16-byte pairs on neighbouring rows;
// where the events go is the data's, so the atomics are the scattered shape of the guide, not the contiguous one: 32 bytes of atomic
// traffic per event and window, on planes that fit the L2 / MALL (11.5 MB per image at 260 x 346, steps 9).
// Workspace cap: a chunk is at most EDI_MAX_CHUNK = 16 images, i.e. 16 (steps - 1) h w 16 bytes of planes (184 MB at 260 x 346, steps 9);
// evd_edi_prior works through more images chunk by chunk and accepts any workspace that holds one image.
#include "evd_common.h"

namespace evd {

constexpr int EDI_MAX_CHUNK = 16;
constexpr int EDI_MAX_STEPS = 65;                       // k_edi_prior_deblur stages steps - 1 floats per thread in LDS (128 threads: 32 KB)
constexpr int EDI_FRAC_BITS = 40;
constexpr double EDI_Q = 1.0 / (double)(1ll << EDI_FRAC_BITS);
constexpr int EDI_SPLAT_BLOCKS = 512;                   // grid-stride blocks per image
constexpr int EDI_DEBLUR_THREADS = 128;

typedef unsigned long long u64;

// time column of the [N, 4] table: row stride 32 bytes
__device__ __forceinline__ double edi_t(const double* __restrict__ events, long e) { return events[e * 4 + 1]; }

__global__ __launch_bounds__(256) void k_edi_windows(const double* __restrict__ events, long N, const double* __restrict__ boundaries, long nb,
                                                     long long* __restrict__ left, long long* __restrict__ right,
                                                     long long* __restrict__ left_out, long long* __restrict__ right_out) {
    const long k = blockIdx.x * 256L + threadIdx.x;
    if (k >= nb) return;
    const double b = boundaries[k];
    long lo = 0, hi = N;
    while (lo < hi) {                                    // first index with t >= b
        const long mid = (lo + hi) >> 1;
        if (edi_t(events, mid) < b) lo = mid + 1; else hi = mid;
    }
    const long l = lo;
    hi = N;
    while (lo < hi) {                                    // first index with t > b
        const long mid = (lo + hi) >> 1;
        if (!(b < edi_t(events, mid))) lo = mid + 1; else hi = mid;
    }
    left[k] = l;
    right[k] = lo;
    if (left_out) { left_out[k] = l; right_out[k] = lo; }
}

// acc: [chunk][steps - 1][2 (pos, neg)][h w] signed 64-bit sums in units of EDI_Q
__global__ __launch_bounds__(256) void k_edi_prior_splat(const double* __restrict__ events, const double* __restrict__ id_to_coords, long n_coords,
                                                         const long long* __restrict__ left, const long long* __restrict__ right, int steps, int h, int w,
                                                         u64* __restrict__ acc, int* __restrict__ bad_id) {
    extern __shared__ long long s_win[];                 // left[i, 0 .. steps), right[i, 0 .. steps)
    const int img = blockIdx.y;
    for (int k = threadIdx.x; k < steps; k += 256) {
        s_win[k] = left[(long)img * steps + k];
        s_win[steps + k] = right[(long)img * steps + k];
    }
    __syncthreads();
    const long long* sl = s_win;
    const long long* sr = s_win + steps;
    const long e0 = sl[0], e1 = sr[steps - 1];
    const long hw = (long)h * w;
    u64* acc_img = acc + (long)img * (steps - 1) * 2 * hw;
    for (long e = e0 + blockIdx.x * 256L + threadIdx.x; e < e1; e += (long)gridDim.x * 256L) {
        const double idf = events[e * 4];
        if (!(idf >= 0.0 && idf < (double)n_coords)) {   // (a NaN id fails both)
            if (bad_id) *bad_id = 1;
            continue;
        }
        const long id = (long)idf;
        const double xv = id_to_coords[2 * id], yv = id_to_coords[2 * id + 1];
        const int plane = events[e * 4 + 2] > 0.0 ? 0 : 1;
        // the four floor / ceil taps (utils/edi.py:17-39): an integer coordinate contributes through its floor case only
        long pix[4];
        u64 q[4];
        int nt = 0;
#pragma unroll
        for (int xr = 0; xr < 2; ++xr)
#pragma unroll
            for (int yr = 0; yr < 2; ++yr) {
                const double xf = xr ? ceil(xv) : floor(xv), yf = yr ? ceil(yv) : floor(yv);
                const bool ok = (xf != xv || xr == 0) && (yf != yv || yr == 0) && xf < (double)w && yf < (double)h && xf >= 0.0 && yf >= 0.0;
                const double kx = fmax(0.0, 1.0 - fabs(xf - xv)), ky = fmax(0.0, 1.0 - fabs(yf - yv));
                pix[xr * 2 + yr] = ok ? (long)yf * w + (long)xf : -1;
                q[xr * 2 + yr] = (u64)llrint(kx * ky * (double)(1ll << EDI_FRAC_BITS));
                nt += ok;
            }
        if (nt == 0) continue;
        for (int j = 0; j < steps - 1; ++j) {
            if (!(sl[j] <= e && e < sr[j + 1])) continue;
            u64* pl = acc_img + ((long)j * 2 + plane) * hw;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (pix[k] >= 0 && q[k]) atomicAdd(pl + pix[k], q[k]);
        }
    }
}

// utils/edi.py:69, 73-95 per pixel; blockIdx.y = image of the chunk
__global__ __launch_bounds__(EDI_DEBLUR_THREADS) void k_edi_prior_deblur(const float* __restrict__ images, const long long* __restrict__ acc, int steps,
                                                                         long hw, float c_pos, float c_neg, float* __restrict__ prior) {
    extern __shared__ float s_bii[];                     // [steps - 1][EDI_DEBLUR_THREADS]
    const long px = blockIdx.x * (long)EDI_DEBLUR_THREADS + threadIdx.x;
    if (px >= hw) return;
    const int img = blockIdx.y, T = EDI_DEBLUR_THREADS, N = (steps - 1) / 2;
    const long long* a = acc + (long)img * (steps - 1) * 2 * hw + px;
    float* b = s_bii + threadIdx.x;
    for (int j = 0; j < steps - 1; ++j) {
        const float pos = (float)((double)a[((long)j * 2) * hw] * EDI_Q), neg = (float)((double)a[((long)j * 2 + 1) * hw] * EDI_Q);
        b[j * T] = pos * c_pos - neg * c_neg;
    }
    // sum_k exp(E_k), k ascending as np.exp(images).sum(axis=0) adds them: the left part, the frame at f, the right part
    float s = 0.f;
    for (int i = 0; i < N; ++i) {
        float e = 0.f;
        for (int j = i; j < N; ++j) e += b[j * T];       // bii[i:N].sum(axis=0)
        s += expf(-e);
    }
    s += 1.f;
    for (int i = 0; i < N; ++i) {
        float e = 0.f;
        for (int j = N; j <= N + i; ++j) e += b[j * T];  // bii[N:N + 1 + i].sum(axis=0)
        s += expf(e);
    }
    const float* im = images + ((long)img * hw + px) * 3;
    float* o = prior + ((long)img * hw + px) * 3;
    const float fs = (float)steps;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = fs * im[c] / s;
}

// ---- the per-image forms: one blurry grey image, float sums
// utils/edi.py:73-95: E_k = -sum_{j=k}^{N-1} bii_j (k<N), 0 (k=N), +sum_{j=N}^{k-1} bii_j (k>N); sharp = (2N+1) blurry / sum exp(E_k)
__global__ void k_edi_deblur(const float* __restrict__ blurry, const float* __restrict__ bii, int steps, long npix,
                             float* __restrict__ sharp) {
    const long px = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (px >= npix) return;
    const int N = (steps - 1) / 2;
    float s = 1.f;       // exp(0) of the frame at f
    float run = 0.f;
    // left part: E_i = -(bii_i + ... + bii_{N-1}); accumulate in the reference's order (i ascending inside each sum)
    for (int i = 0; i < N; ++i) {
        float e = 0.f;
        for (int j = i; j < N; ++j) e += bii[(long)j * npix + px];
        s += expf(-e);
    }
    for (int i = 0; i < N; ++i) {
        run += bii[(long)(N + i) * npix + px];
        s += expf(run);
    }
    sharp[px] = (float)(2 * N + 1) * blurry[px] / s;
}

// utils/edi.py:7-41,44-70: bilinear sub-pixel splat of +-1 events, grey sensor
__global__ void k_edi_splat(const float* __restrict__ x, const float* __restrict__ y, const signed char* __restrict__ p, long n,
                            int w, int h, float c_pos, float c_neg, float* __restrict__ image) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float xv = x[i], yv = y[i];
    const float sc = p[i] > 0 ? c_pos : -c_neg;
#pragma unroll
    for (int xr = 0; xr < 2; ++xr)
#pragma unroll
        for (int yr = 0; yr < 2; ++yr) {
            const float xf = xr ? ceilf(xv) : floorf(xv), yf = yr ? ceilf(yv) : floorf(yv);
            // (a tap left of / above the frame is dropped: the reference's negative index wraps to the opposite edge, an indexing artefact)
            if (!((xf != xv || xr == 0) && (yf != yv || yr == 0) && xf < (float)w && yf < (float)h && xf >= 0.f && yf >= 0.f)) continue;
            const float kx = fmaxf(0.f, 1.f - fabsf(xf - xv)), ky = fmaxf(0.f, 1.f - fabsf(yf - yv));
            atomicAdd(image + (long)yf * w + (long)xf, sc * (kx * ky));
        }
}

static inline size_t edi_plane_bytes(int steps, int h, int w) { return (size_t)(steps - 1) * h * w * 16; }
// workspace of evd_edi_prior at a chunk of c images: the window bounds [c, steps] x 2 | the accumulator planes, which end the workspace unpadded
struct EdiWs { long long *left, *right; u64* acc; };
static const size_t EDI_WS_SLACK = 256;     // alignment slack for an unaligned caller pointer
static size_t edi_layout(int c, int steps, int h, int w, void* workspace, EdiWs* L) {
    Workspace ws(workspace);
    L->left = ws.take<long long>((size_t)c * steps); L->right = ws.take<long long>((size_t)c * steps); L->acc = ws.take<u64>(0);
    return ws.used() + (size_t)c * edi_plane_bytes(steps, h, w) + EDI_WS_SLACK;
}

}  // namespace evd

using namespace evd;

extern "C" {

size_t evd_edi_prior_workspace_bytes(int n_img, int steps, int h, int w) {
    if (n_img < 1 || steps < 3 || !(steps & 1) || steps > EDI_MAX_STEPS || h < 1 || w < 1 || (long)h * w >= (1L << 31)) return 0;
    EdiWs L;
    return edi_layout(n_img < EDI_MAX_CHUNK ? n_img : EDI_MAX_CHUNK, steps, h, w, nullptr, &L);
}

int evd_edi_prior(const double* events, long N, const double* id_to_coords, long n_coords, const double* boundaries, const float* images,
                  int n_img, int steps, int h, int w, float c_pos, float c_neg, float* prior_out, long long* windows_out, int* bad_id,
                  void* workspace, size_t workspace_bytes, void* stream) {
    EVD_REQUIRE(steps >= 3 && (steps & 1) && steps <= EDI_MAX_STEPS, "evd_edi_prior: steps %d (odd, 3 .. %d)", steps, EDI_MAX_STEPS);
    EVD_REQUIRE(N >= 0 && n_coords >= 0 && n_img >= 1 && h >= 1 && w >= 1 && (long)h * w < (1L << 31) && n_img < 65536,
                "evd_edi_prior: bad sizes N=%ld n_coords=%ld n_img=%d h=%d w=%d", N, n_coords, n_img, h, w);
    EVD_REQUIRE(boundaries && images && prior_out && (N == 0 || (events && id_to_coords)), "evd_edi_prior: null argument");
    EdiWs L;
    const size_t need = edi_layout(1, steps, h, w, workspace, &L);
    EVD_REQUIRE(workspace && workspace_bytes >= need, "evd_edi_prior: workspace %zu < %zu bytes (one image)", workspace_bytes, need);
    int chunk = n_img < EDI_MAX_CHUNK ? n_img : EDI_MAX_CHUNK;
    while (edi_layout(chunk, steps, h, w, workspace, &L) > workspace_bytes) --chunk;       // >= 1: checked above; L is the layout at the chunk that fits
    hipStream_t st = as_stream(stream);
    const long hw = (long)h * w;
    long long *left = L.left, *right = L.right; u64* acc = L.acc;
    if (bad_id) EVD_HIP(hipMemsetAsync(bad_id, 0, sizeof(int), st));
    for (int c0 = 0; c0 < n_img; c0 += chunk) {
        const int cn = n_img - c0 < chunk ? n_img - c0 : chunk;
        const long nb = (long)cn * steps;
        EVD_HIP(hipMemsetAsync(acc, 0, (size_t)cn * edi_plane_bytes(steps, h, w), st));
        k_edi_windows<<<(unsigned)cdiv(nb, 256L), 256, 0, st>>>(events, N, boundaries + (long)c0 * steps, nb, left, right,
                                                               windows_out ? windows_out + (long)c0 * steps : nullptr,
                                                               windows_out ? windows_out + ((long)n_img + c0) * steps : nullptr);
        if (N > 0)
            k_edi_prior_splat<<<dim3(EDI_SPLAT_BLOCKS, cn), 256, 2 * steps * sizeof(long long), st>>>(events, id_to_coords, n_coords, left, right, steps, h, w, acc,
                                                                                                     bad_id);
        k_edi_prior_deblur<<<dim3((unsigned)cdiv(hw, (long)EDI_DEBLUR_THREADS), cn), EDI_DEBLUR_THREADS, (size_t)(steps - 1) * EDI_DEBLUR_THREADS * sizeof(float), st>>>(
            images + (long)c0 * hw * 3, (const long long*)acc, steps, hw, c_pos, c_neg, prior_out + (long)c0 * hw * 3);
        EVD_LAUNCH_CHECK();
    }
    return EVD_OK;
}

int evd_edi_deblur(const float* blurry, const float* bii, int steps, long npix, float* sharp, void* stream) {
    EVD_REQUIRE(blurry && bii && sharp && steps >= 3 && (steps & 1) && npix >= 0, "evd_edi_deblur: steps must be odd >= 3");
    if (npix == 0) return EVD_OK;
    k_edi_deblur<<<cdiv(npix, 256), 256, 0, as_stream(stream)>>>(blurry, bii, steps, npix, sharp);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int evd_edi_bii_image(const float* x, const float* y, const signed char* p, long n, int w, int h,
                      float c_pos, float c_neg, float* image, void* stream) {
    EVD_REQUIRE(image && w > 0 && h > 0 && n >= 0, "evd_edi_bii_image: bad arguments");
    EVD_HIP(hipMemsetAsync(image, 0, sizeof(float) * (size_t)w * h, as_stream(stream)));
    if (n == 0) return EVD_OK;
    k_edi_splat<<<cdiv(n, 256), 256, 0, as_stream(stream)>>>(x, y, p, n, w, h, c_pos, c_neg, image);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

}  // extern "C"
