// 8-bit pictures of frame stacks on the device: the arithmetic between render_path and the image / video / logger calls of the test-set,
// video and render-only passes (reference run_nerf.py:374-389, 663-679, 726-732) -- depth pictures, error maps, the video's normalised RGB.
// The reference copies the float32 frames to the host and lets NumPy make several full-size temporaries; here a picture kind is two calls:
//   k_frame_range         min and max of the VALUE of every element of a slice (the whole stack, or one frame): a workgroup takes FR_EPB
//                         consecutive values, folds them with fminf / fmaxf (a NaN is skipped) and writes one (min, max) partial
//   k_frame_range_finish  one workgroup per slice folds the slice's partials in a fixed order and writes (lo, hi) to device memory
//   k_frame_map           the same walk; reads (lo, hi) from device memory (no host synchronisation between the launches), forms
//                         y = v / hi or (v - lo) / (hi - lo), g = to8b(y), and stores g or the three bytes lut[255 - g] of a table in LDS
//   k_frame_colormap      the bare lookup lut[g] of a uint8 picture
// The value of an element comes from ONE function both walks call (frame_value: x, 1 - x, or the mean squared error of a pixel's three
// channels, which is never stored), so range and map cannot disagree.  Every step is a single correctly rounded float32 operation in the
// order NumPy uses (build.py compiles with -ffp-contract=off; IEEE division, no reciprocal): the bytes are defined bit for bit.
// No floating-point atomics: two runs give the same bits.
// Walk of a slice: its first `head` values (0..3, up to the first 16-byte boundary of the source) and its last n % 4 go one by one, the
// groups of 4 between them as 16-byte loads (SQERR: 3 + 3 of them, 4 pixels) and one 4-byte store (with a table: three), where every
// pointer of the slice is aligned at the head; a slice whose pointers are not -- frames of an odd size start anywhere -- goes one by one.
// Memory bound: 4 (plain, inverted) or 24 (error) bytes read per value in each of the two walks, 1 or 3 bytes written.
#include "evd_common.h"

#pragma clang fp contract(off)          // as the build's -ffp-contract=off: a fused multiply-add would change the error map's bits

namespace evd {

constexpr int FR_THREADS = 256;
constexpr int FR_ITERS = 8;
constexpr long FR_EPB = (long)FR_THREADS * 4 * FR_ITERS;      // values per workgroup
constexpr int FR_FINISH_THREADS = 1024;

// a slice's geometry, the same for the two walks: blockIdx.x = slice * bps + b
struct FrameWalk {
    const float* x;
    const float* y;
    long n;             // values per slice
    long bps;           // workgroups per slice: cdiv(n, FR_EPB)
};

// the value of element i of a slice (xs, ys: the slice's sources)
template <int SRC>
__device__ __forceinline__ float frame_value(const float* __restrict__ xs, const float* __restrict__ ys, long i) {
    if (SRC == EVD_FRAME_SRC_PLAIN) return xs[i];
    if (SRC == EVD_FRAME_SRC_INVERT) return 1.f - xs[i];
    const float d0 = xs[3 * i] - ys[3 * i], d1 = xs[3 * i + 1] - ys[3 * i + 1], d2 = xs[3 * i + 2] - ys[3 * i + 2];
    return ((d0 * d0 + d1 * d1) + d2 * d2) / 3.f;           // np.mean(-1) of a float32 [..., 3] array: ((a0 + a1) + a2) / 3
}

// the values of elements i .. i + 3, i a multiple of 4 past the head: 16-byte loads
template <int SRC>
__device__ __forceinline__ void frame_value4(const float* __restrict__ xs, const float* __restrict__ ys, long i, float v[4]) {
    if (SRC != EVD_FRAME_SRC_SQERR) {
        const float4 a = *reinterpret_cast<const float4*>(xs + i);
        v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
        if (SRC == EVD_FRAME_SRC_INVERT) {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = 1.f - v[k];
        }
    } else {
        float4 p4[3], t4[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            p4[k] = *reinterpret_cast<const float4*>(xs + 3 * i + 4 * k);
            t4[k] = *reinterpret_cast<const float4*>(ys + 3 * i + 4 * k);
        }
        const float* p = reinterpret_cast<const float*>(p4);
        const float* t = reinterpret_cast<const float*>(t4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float d0 = p[3 * k] - t[3 * k], d1 = p[3 * k + 1] - t[3 * k + 1], d2 = p[3 * k + 2] - t[3 * k + 2];
            v[k] = ((d0 * d0 + d1 * d1) + d2 * d2) / 3.f;
        }
    }
}

// values in front of the first 16-byte boundary of the slice's source: floats for a plain source; for pixels of 3 floats at phase a
// (a + 3 h = 0 mod 4 <=> h = a mod 4)
template <int SRC>
__device__ __forceinline__ int frame_head(const float* xs) {
    const int a = (int)(((uintptr_t)xs >> 2) & 3);
    return SRC == EVD_FRAME_SRC_SQERR ? a : (4 - a) & 3;
}

// The walk both kernels share.  f1(i, v) takes one value, f4(i, v[4]) the four values i .. i + 3 of an aligned group; `vec`: the groups
// may be loaded (and by f4 stored) as vectors.  Workgroup b of the slice covers values head + [b FR_EPB, (b + 1) FR_EPB), workgroup 0 the
// head as well; every index is checked against n.
template <int SRC, class F1, class F4>
__device__ __forceinline__ void frame_walk(const float* __restrict__ xs, const float* __restrict__ ys, long n, long b, int head, bool vec, F1 f1, F4 f4) {
    if (b == 0 && (int)threadIdx.x < head && (long)threadIdx.x < n) f1((long)threadIdx.x, frame_value<SRC>(xs, ys, (long)threadIdx.x));
    const long g0 = head + b * FR_EPB + (long)threadIdx.x * 4;
#pragma unroll 2
    for (int it = 0; it < FR_ITERS; ++it) {
        const long g = g0 + (long)it * FR_THREADS * 4;
        if (g >= n) break;
        if (vec && g + 4 <= n) {
            float v[4];
            frame_value4<SRC>(xs, ys, g, v);
            f4(g, v);
        } else {
            for (long j = g; j < n && j < g + 4; ++j) f1(j, frame_value<SRC>(xs, ys, j));
        }
    }
}

__device__ __forceinline__ float fr_wave_min(float v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float fr_wave_max(float v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// partials [slices * bps][2]
template <int SRC>
__global__ __launch_bounds__(FR_THREADS) void k_frame_range(FrameWalk w, float* __restrict__ partials) {
    __shared__ float s_red[FR_THREADS / 64][2];
    const long s = blockIdx.x / w.bps, b = blockIdx.x - s * w.bps;
    const long off = s * w.n * (SRC == EVD_FRAME_SRC_SQERR ? 3 : 1);
    const float* xs = w.x + off;
    const float* ys = SRC == EVD_FRAME_SRC_SQERR ? w.y + off : nullptr;
    const int head = frame_head<SRC>(xs);
    const bool vec = SRC != EVD_FRAME_SRC_SQERR || (((uintptr_t)xs ^ (uintptr_t)ys) & 15) == 0;
    float mn = INFINITY, mx = -INFINITY;
    frame_walk<SRC>(
        xs, ys, w.n, b, head, vec, [&](long, float v) { mn = fminf(mn, v), mx = fmaxf(mx, v); },
        [&](long, const float v[4]) {
#pragma unroll
            for (int k = 0; k < 4; ++k) mn = fminf(mn, v[k]), mx = fmaxf(mx, v[k]);
        });
    mn = fr_wave_min(mn);
    mx = fr_wave_max(mx);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) s_red[wave][0] = mn, s_red[wave][1] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < FR_THREADS / 64; ++k) mn = fminf(mn, s_red[k][0]), mx = fmaxf(mx, s_red[k][1]);
        partials[2 * (long)blockIdx.x] = mn;
        partials[2 * (long)blockIdx.x + 1] = mx;
    }
}

// one workgroup per slice: thread t takes partials t, t + FR_FINISH_THREADS, ..., then a butterfly per wavefront and the wavefronts in order
// (a stack of 120 frames of 400 x 400 x 3 under scope ALL has 7032 partials: 7 dependent steps per thread; a single wavefront would need 110)
__global__ __launch_bounds__(FR_FINISH_THREADS) void k_frame_range_finish(const float* __restrict__ partials, long bps, float* __restrict__ range) {
    __shared__ float s_red[FR_FINISH_THREADS / 64][2];
    const float* p = partials + 2 * (long)blockIdx.x * bps;
    float mn = INFINITY, mx = -INFINITY;
    for (long t = threadIdx.x; t < bps; t += FR_FINISH_THREADS) mn = fminf(mn, p[2 * t]), mx = fmaxf(mx, p[2 * t + 1]);
    mn = fr_wave_min(mn);
    mx = fr_wave_max(mx);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) s_red[wave][0] = mn, s_red[wave][1] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < FR_FINISH_THREADS / 64; ++k) mn = fminf(mn, s_red[k][0]), mx = fmaxf(mx, s_red[k][1]);
        range[2 * (long)blockIdx.x] = mn, range[2 * (long)blockIdx.x + 1] = mx;
    }
}

// out [slices * n] or, with LUT, [slices * n, 3]
template <int SRC, bool LUT>
__global__ __launch_bounds__(FR_THREADS) void k_frame_map(FrameWalk w, const float* __restrict__ range, int subtract_lo, const unsigned char* __restrict__ lut,
                                                          unsigned char* __restrict__ out) {
    __shared__ unsigned char s_lut[LUT ? 768 : 4];
    if (LUT) {
        for (int i = threadIdx.x; i < 768; i += FR_THREADS) s_lut[i] = lut[i];
        __syncthreads();
    }
    const long s = blockIdx.x / w.bps, b = blockIdx.x - s * w.bps;
    const long off = s * w.n * (SRC == EVD_FRAME_SRC_SQERR ? 3 : 1);
    const float* xs = w.x + off;
    const float* ys = SRC == EVD_FRAME_SRC_SQERR ? w.y + off : nullptr;
    unsigned char* os = out + s * w.n * (LUT ? 3 : 1);
    const int head = frame_head<SRC>(xs);
    const bool vec = (SRC != EVD_FRAME_SRC_SQERR || (((uintptr_t)xs ^ (uintptr_t)ys) & 15) == 0) && ((uintptr_t)(os + (long)head * (LUT ? 3 : 1)) & 3) == 0;
    const float lo = subtract_lo ? range[2 * s] : 0.f, hi = range[2 * s + 1];
    const float den = subtract_lo ? hi - lo : hi;
    const bool flat = subtract_lo ? hi == lo : hi == 0.f;                 // a constant slice: grey level 0 (the reference divides by zero)
    auto grey = [&](float v) -> unsigned {
        if (flat) return 0u;
        return to8b_u8(subtract_lo ? (v - lo) / den : v / den);           // evd_to8b's function (evd_common.h)
    };
    frame_walk<SRC>(
        xs, ys, w.n, b, head, vec,
        [&](long i, float v) {
            const unsigned g = grey(v);
            if (LUT) {
#pragma unroll
                for (int c = 0; c < 3; ++c) os[3 * i + c] = s_lut[(255u - g) * 3 + c];
            } else {
                os[i] = (unsigned char)g;
            }
        },
        [&](long i, const float v[4]) {
            if (LUT) {
                unsigned char q[12];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned r = (255u - grey(v[k])) * 3;
#pragma unroll
                    for (int c = 0; c < 3; ++c) q[3 * k + c] = s_lut[r + c];
                }
                unsigned* o = reinterpret_cast<unsigned*>(os + 3 * i);
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    o[k] = (unsigned)q[4 * k] | ((unsigned)q[4 * k + 1] << 8) | ((unsigned)q[4 * k + 2] << 16) | ((unsigned)q[4 * k + 3] << 24);
            } else {
                *reinterpret_cast<unsigned*>(os + i) = grey(v[0]) | (grey(v[1]) << 8) | (grey(v[2]) << 16) | (grey(v[3]) << 24);
            }
        });
}

// the bare table lookup: out[i] = lut[g[i]], 4 pictures' bytes per thread (`vec`: g and out 4-byte aligned; the last n % 4 go one by one)
__global__ __launch_bounds__(FR_THREADS) void k_frame_colormap(const unsigned char* __restrict__ g, long n, const unsigned char* __restrict__ lut,
                                                               unsigned char* __restrict__ out, int vec) {
    __shared__ unsigned char s_lut[768];
    for (int i = threadIdx.x; i < 768; i += FR_THREADS) s_lut[i] = lut[i];
    __syncthreads();
    const long i = ((long)blockIdx.x * FR_THREADS + threadIdx.x) * 4;
    if (i >= n) return;
    if (vec && i + 4 <= n) {
        const unsigned v = *reinterpret_cast<const unsigned*>(g + i);
        unsigned char q[12];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int c = 0; c < 3; ++c) q[3 * k + c] = s_lut[((v >> (8 * k)) & 255u) * 3 + c];
        }
        unsigned* o = reinterpret_cast<unsigned*>(out + 3 * i);
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = (unsigned)q[4 * k] | ((unsigned)q[4 * k + 1] << 8) | ((unsigned)q[4 * k + 2] << 16) | ((unsigned)q[4 * k + 3] << 24);
    } else {
        for (long j = i; j < n && j < i + 4; ++j) {
#pragma unroll
            for (int c = 0; c < 3; ++c) out[3 * j + c] = s_lut[(unsigned)g[j] * 3 + c];
        }
    }
}

// the walk's geometry for the entries: a stack under scope ALL is one slice
static inline bool fr_geometry(int n_frames, long per_frame, int scope, long* slices, long* n, long* bps) {
    if (n_frames <= 0 || per_frame <= 0 || per_frame >= (1L << 40)) return false;
    const long total = (long)n_frames * per_frame;
    if (total * 3 >= (1L << 40)) return false;              // the largest offset either walk forms: a pixel's floats, a table picture's bytes
    *slices = scope == EVD_FRAME_SCOPE_ALL ? 1 : n_frames;
    *n = scope == EVD_FRAME_SCOPE_ALL ? total : per_frame;
    *bps = cdiv(*n, FR_EPB);
    return *slices * *bps < (1L << 31);
}

static inline bool fr_tags_ok(int source, int scope) {
    return (source == EVD_FRAME_SRC_PLAIN || source == EVD_FRAME_SRC_INVERT || source == EVD_FRAME_SRC_SQERR) &&
           (scope == EVD_FRAME_SCOPE_ALL || scope == EVD_FRAME_SCOPE_FRAME);
}

}  // namespace evd

using namespace evd;

extern "C" {

size_t evd_frame_workspace_bytes(int n_frames, long per_frame, int scope) {
    long slices, n, bps;
    if (!fr_tags_ok(EVD_FRAME_SRC_PLAIN, scope) || !fr_geometry(n_frames, per_frame, scope, &slices, &n, &bps)) return 0;
    return (size_t)(slices * bps) * 2 * sizeof(float) + 256;
}

int evd_frame_range(const float* x, const float* y, int source, int scope, int n_frames, long per_frame, float* range, void* workspace,
                    size_t workspace_bytes, void* stream) {
    EVD_REQUIRE(fr_tags_ok(source, scope), "evd_frame_range: unknown source %d or scope %d", source, scope);
    long slices, n, bps;
    EVD_REQUIRE(fr_geometry(n_frames, per_frame, scope, &slices, &n, &bps), "evd_frame_range: bad sizes n_frames=%d per_frame=%ld", n_frames, per_frame);
    EVD_REQUIRE(x && range && (source != EVD_FRAME_SRC_SQERR || y), "evd_frame_range: null argument");
    const size_t need = (size_t)(slices * bps) * 2 * sizeof(float) + 256;
    EVD_REQUIRE(workspace && workspace_bytes >= need, "evd_frame_range: workspace %zu < %zu bytes", workspace_bytes, need);
    hipStream_t st = as_stream(stream);
    float* partials = (float*)ws_align_ptr(workspace);
    const FrameWalk w = {x, y, n, bps};
    const unsigned grid = (unsigned)(slices * bps);
    if (source == EVD_FRAME_SRC_PLAIN) k_frame_range<EVD_FRAME_SRC_PLAIN><<<grid, FR_THREADS, 0, st>>>(w, partials);
    else if (source == EVD_FRAME_SRC_INVERT) k_frame_range<EVD_FRAME_SRC_INVERT><<<grid, FR_THREADS, 0, st>>>(w, partials);
    else k_frame_range<EVD_FRAME_SRC_SQERR><<<grid, FR_THREADS, 0, st>>>(w, partials);
    k_frame_range_finish<<<(unsigned)slices, FR_FINISH_THREADS, 0, st>>>(partials, bps, range);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int evd_frame_map(const float* x, const float* y, int source, int scope, int n_frames, long per_frame, const float* range, int subtract_lo,
                  const unsigned char* lut, unsigned char* out, void* stream) {
    EVD_REQUIRE(fr_tags_ok(source, scope), "evd_frame_map: unknown source %d or scope %d", source, scope);
    long slices, n, bps;
    EVD_REQUIRE(fr_geometry(n_frames, per_frame, scope, &slices, &n, &bps), "evd_frame_map: bad sizes n_frames=%d per_frame=%ld", n_frames, per_frame);
    EVD_REQUIRE(x && range && out && (source != EVD_FRAME_SRC_SQERR || y), "evd_frame_map: null argument");
    hipStream_t st = as_stream(stream);
    const FrameWalk w = {x, y, n, bps};
    const unsigned grid = (unsigned)(slices * bps);
    const int sub = subtract_lo ? 1 : 0;
#define EVD_FRAME_MAP(SRC)                                                                            \
    do {                                                                                              \
        if (lut) k_frame_map<SRC, true><<<grid, FR_THREADS, 0, st>>>(w, range, sub, lut, out);        \
        else k_frame_map<SRC, false><<<grid, FR_THREADS, 0, st>>>(w, range, sub, lut, out);           \
    } while (0)
    if (source == EVD_FRAME_SRC_PLAIN) EVD_FRAME_MAP(EVD_FRAME_SRC_PLAIN);
    else if (source == EVD_FRAME_SRC_INVERT) EVD_FRAME_MAP(EVD_FRAME_SRC_INVERT);
    else EVD_FRAME_MAP(EVD_FRAME_SRC_SQERR);
#undef EVD_FRAME_MAP
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int evd_frame_colormap(const unsigned char* g, long n, const unsigned char* lut, unsigned char* out, void* stream) {
    EVD_REQUIRE(n >= 0 && n * 3 < (1L << 40), "evd_frame_colormap: bad size n=%ld", n);
    if (n == 0) return EVD_OK;
    EVD_REQUIRE(g && lut && out, "evd_frame_colormap: null argument");
    const int vec = (((uintptr_t)g | (uintptr_t)out) & 3) == 0;
    k_frame_colormap<<<(unsigned)cdiv(cdiv(n, 4L), (long)FR_THREADS), FR_THREADS, 0, as_stream(stream)>>>(g, n, lut, out, vec);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

}  // extern "C"
