// k_numerics_flags, the NaN / Inf guard of the render outputs, and nothing else: the rest of the render path lives by concern in
// kernels_rays.hip (ray front end), kernels_composite.hip (compositing scan) and kernels_sample_pdf.hip (inverse-CDF resampling).
#include <algorithm>
#include <cstdint>

#include "evd_common.h"
#include "wave_ops.h"

namespace evd {

// reference networks/renderer.py:259-263: the per-key isnan / isinf guard of render_rays (two host syncs per key there).
// Here: one launch over all keys, flags[k] |= 1 (NaN) | 2 (Inf), no sync; the caller reads the word when it wants to.
constexpr int NUMERICS_MAX_KEYS = 16;
struct NumericsKeys {
    const float* p[NUMERICS_MAX_KEYS];
    long n[NUMERICS_MAX_KEYS];
    int keys;
};
__global__ void k_numerics_flags(const NumericsKeys a, unsigned* __restrict__ flags) {
    const int k = blockIdx.y;
    if (k >= a.keys) return;
    const float* __restrict__ x = a.p[k];
    const long n = a.n[k];
    unsigned f = 0;
    // exponent all ones: mantissa != 0 -> NaN, == 0 -> Inf
    auto look = [&](float v) {
        const unsigned u = __float_as_uint(v);
        if ((u & 0x7f800000u) == 0x7f800000u) f |= (u & 0x007fffffu) ? 1u : 2u;
    };
    const long stride = (long)gridDim.x * blockDim.x;
    long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if ((reinterpret_cast<uintptr_t>(x) & 15) == 0) {
        const float4* __restrict__ x4 = reinterpret_cast<const float4*>(x);
        for (long j = i; j < n / 4; j += stride) {
            const float4 v = x4[j];
            look(v.x); look(v.y); look(v.z); look(v.w);
        }
        for (long j = (n / 4) * 4 + i; j < n; j += stride) look(x[j]);
    } else {
        for (long j = i; j < n; j += stride) look(x[j]);
    }
    f = wave_or(f);
    if ((threadIdx.x & 63) == 0 && f) atomicOr(&flags[k], f);
}

}  // namespace evd

extern "C" {

int evd_numerics_flags(const float* const* ptrs, const long* counts, int n_keys, unsigned* flags, void* stream) {
    using namespace evd;
    EVD_REQUIRE(n_keys >= 0 && n_keys <= NUMERICS_MAX_KEYS, "evd_numerics_flags: n_keys %d (max %d)", n_keys, NUMERICS_MAX_KEYS);
    if (n_keys == 0) return EVD_OK;
    EVD_REQUIRE(ptrs && counts && flags, "evd_numerics_flags: null argument");
    NumericsKeys a{};
    a.keys = n_keys;
    long most = 0;
    for (int k = 0; k < n_keys; ++k) {
        EVD_REQUIRE(counts[k] >= 0 && (ptrs[k] || counts[k] == 0), "evd_numerics_flags: key %d is null", k);
        a.p[k] = ptrs[k];
        a.n[k] = counts[k];
        most = counts[k] > most ? counts[k] : most;
    }
    EVD_HIP(hipMemsetAsync(flags, 0, sizeof(unsigned) * n_keys, as_stream(stream)));
    const int bx = (int)std::min<long>(std::max<long>(cdiv(most, 256 * 16), 1), 1024);
    hipLaunchKernelGGL(k_numerics_flags, dim3(bx, n_keys), dim3(256), 0, as_stream(stream), a, flags);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

}  // extern "C"
