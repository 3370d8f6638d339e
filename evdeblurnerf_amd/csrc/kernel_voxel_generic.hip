// PDRF level of any depth, width and geo size (reference networks/pdrf/voxnerf.py:48-82,210-221,240-254): the per-sample part of
// VoxelNeRFBase.forward with num_layers / num_layers_color 1..4, hidden_dim 64 / 128 / 256, geo_feat_dim 1..128 and 16..64 feature
// channels, in the four arithmetic modes of k_voxel_mlp on the same layer<> machinery (mlp_device.h).
//
// A kernel of its own and not a switch in k_voxel_mlp: the standard levels' code objects stay what they are.  Templated on
// <PREC, HD, S1, C1>.  S1 / C1 are num_layers == 1 / num_layers_color == 1, where a network is its head alone: with both forms of a
// network in one body the 256-wide kernels spill (S1: the half-precision ones, 8 - 44 bytes per lane; C1: the split-float16 one, 308).
// The other layer counts, the geo tile count and the feature k-steps are kernel arguments.  Every register array is indexed by an
// unrolled loop variable and the run-time counts only choose between whole layers (block-uniform branches), so nothing is indexed
// dynamically.  Compiled with the MFMAs in VGPR form (build.py): the 256-wide split-float16 kernel has scratch without.
//
// Stream (evd_voxel_create, build_generic): EVERY layer starts on a chunk boundary (FOFF 0, PAD_END), in this order
//   sigma_net.0 .. sigma_net.NS-2    T tiles, ReLU            (input of layer 0: VG_KF feature k-steps + PE_KS encoding k-steps)
//   sigma_net.NS-1, row 0            1 tile: the density
//   sigma_net.NS-1, rows 1..G        gt 1-tile layers, 32 geo channels each, the last one zero padded
//   color_net.0 .. color_net.NC-2    T tiles, ReLU, bias      (input of layer 0: VG_GK geo k-steps + PEV_KS encoding k-steps)
//   color_net.NC-1                   1 tile: the three colour rows
// The feature and geo inputs always take VG_KF / VG_GK k-steps: the positions a level does not have are zero columns of the packed
// weights and zero B fragments.
#include "voxel_generic.h"
#include "mlp_device.h"

namespace evd {

// TRAIN (EVD_PREC_F16X3 only): the training forward -- the same stream, the same layer<> calls in the same order, hence the same raw bit
// for bit -- with the inputs and every layer's output also written as float32 rows of the store p.act (VoxGenStore, voxel_generic.h).
template <int PREC, int HD, bool S1, bool C1, bool TRAIN = false>
__global__ __launch_bounds__(mlp_threads(PREC), is_half_prec(PREC) ? 2 : 1) void k_voxel_mlp_generic(const VoxMlpParams p, const VoxGenShape g) {
    typedef Ops<PREC> O;
    typedef typename O::B B;
    constexpr int NT = mlp_threads(PREC);
    constexpr int T = HD / 32, KS = HD / 16;
    constexpr int K0 = VG_KF + PE_KS, KC = VG_GK + PEV_KS;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 31, h = lane >> 5;
    const long s = (long)blockIdx.x * (NT / 2) + wave * 32 + n;
    const bool valid = s < p.nsamp;
    const long sc = valid ? s : p.nsamp - 1;
    float pts[3], vd[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        pts[c] = p.pts[sc * 3 + c];
        vd[c] = p.viewdirs[(sc / p.S) * p.vd_stride + c];
    }
    const f32x8 zero8 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const VoxGenStore gs(p.nsamp, HD, g.ns, g.nc);
    float* const store = (TRAIN && valid) ? reinterpret_cast<float*>(p.act) : nullptr;        // null: this lane writes no rows
    if (TRAIN && store) {       // the encodings' inputs: lane half 0 the position, half 1 the direction
        const f32x4 v = h ? f32x4{vd[0], vd[1], vd[2], 0.f} : f32x4{pts[0], pts[1], pts[2], 0.f};
        *reinterpret_cast<f32x4*>(store + gs.in() + s * 8 + 4 * h) = v;
    }
    // layer-0 input = cat([fts, PE(pts)])  (voxnerf.py:214): the level's kf natural feature k-steps, zero up to VG_KF, then the PE arrangement
    // (cin, the colour net's input, is filled by the geo tiles; its direction part is encoded after the sigma net: fewer live registers)
    B in0[K0], cin[KC];
    {
        const float* f = p.fts + sc * (long)p.ft_stride + 8 * h;
#pragma unroll
        for (int j = 0; j < VG_KF; ++j) {
            f32x8 v = zero8;
            if (j < g.kf) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(f + 16 * j), b = *reinterpret_cast<const f32x4*>(f + 16 * j + 4);
                v = f32x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
                if (TRAIN && store) {
                    float* o = store + gs.fts() + s * VG_FT_LD + 8 * h + 16 * j;
                    *reinterpret_cast<f32x4*>(o) = a;
                    *reinterpret_cast<f32x4*>(o + 4) = b;
                }
            }
            in0[j] = O::make_b(v);
        }
        B pe[PE_KS];
        encode_b_rt<PREC, PE_KS>(pts, h, p.pe_l, pe);
#pragma unroll
        for (int j = 0; j < PE_KS; ++j) in0[VG_KF + j] = pe[j];
    }
    const float* zero_bias = stage_bias<PREC>(smem, p.bias, p.nbias, tid);      // first 512 floats: zeros (sigma net: bias=False)
    const float* cbias = zero_bias + 32 * 16;
    Stream<PREC> st;
    st.start(p.wstream, smem, p.nchunks, tid);

    // ---- sigma net (voxnerf.py:215-218)
    float sig[16];
    float* const frow = (p.feature && valid) ? p.feature + s * g.G : nullptr;
    // one geo tile: B fragments for the colour net and (frow) the float32 rows, columns past G left alone
    // The stores are lane-dependent branches that end where the block-uniform `t < g.gt` region ends, so the compiler takes the stream's
    // position (merged there) for lane-dependent too; it is the same in every lane, and the DMA needs it in a scalar register.
    float* const grow = (TRAIN && store) ? store + gs.geo() + s * VG_GEO_LD : nullptr;
    auto geo_rows = [&](int t, const float (&x)[16]) {
        if (TRAIN && grow) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (c < g.G) grow[c] = x[r];
            }
        }
        if (frow) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (c < g.G) frow[c] = x[r];
            }
        }
        st.cur = __builtin_amdgcn_readfirstlane(st.cur);
        st.slot = __builtin_amdgcn_readfirstlane(st.slot);
    };
    // the last sigma layer on x: the density tile, then the geo tiles (B fragments for the colour net, float32 rows where asked for)
    auto sigma_head = [&](const auto& x) {
        constexpr int KX = sizeof(x) / sizeof(B);
        layer<PREC, KX, 1, false, OUT_F32, 0, true>(st, x, nullptr, sig, zero_bias, lane, nullptr, HD);
#pragma unroll
        for (int t = 0; t < VG_GT; ++t) {
            if (t < g.gt) {
                float y[16];
                layer<PREC, KX, 1, false, OUT_BOTH, 0, true>(st, x, &cin[2 * t], y, zero_bias, lane, nullptr, HD);
                geo_rows(t, y);
            } else {
                cin[2 * t] = cin[2 * t + 1] = O::make_b(zero8);
            }
        }
    };
    if constexpr (S1) {
        sigma_head(in0);
    } else {
        B hid[KS], nxt[KS];
        float* hrow = (TRAIN && store) ? store + gs.hs(0) + s * HD : nullptr;      // row s of sigma_net.0's output; a layer further: nsp * HD floats
        layer<PREC, K0, T, true, OUT_B, 0, true>(st, in0, hid, nullptr, zero_bias, lane, hrow, HD);
#pragma nounroll
        for (int l = 1; l < g.ns - 1; ++l) {
            if (TRAIN && hrow) hrow += gs.nsp * HD;
            layer<PREC, KS, T, true, OUT_B, 0, true>(st, hid, nxt, nullptr, zero_bias, lane, hrow, HD);
#pragma unroll
            for (int j = 0; j < KS; ++j) hid[j] = nxt[j];
        }
        sigma_head(hid);
    }

    // ---- colour net on cat([h[..., 1:], PE(dirs)]) (voxnerf.py:248-252)
    {
        B dir[PEV_KS];
        encode_b_rt<PREC, PEV_KS>(vd, h, p.pe_lv, dir);
#pragma unroll
        for (int j = 0; j < PEV_KS; ++j) cin[VG_GK + j] = dir[j];
    }
    float col[16];
    auto color_head = [&](const auto& x, const float* b) {
        constexpr int KX = sizeof(x) / sizeof(B);
        layer<PREC, KX, 1, false, OUT_F32, 0, true>(st, x, nullptr, col, b, lane, nullptr, HD);
    };
    if constexpr (C1) {
        color_head(cin, cbias);
    } else {
        B c[KS], nxt[KS];
        const float* b = cbias;
        float* crow = (TRAIN && store) ? store + gs.hc(0) + s * HD : nullptr;
        layer<PREC, KC, T, true, OUT_B, 0, true>(st, cin, c, nullptr, b, lane, crow, HD);
        b += 32 * T;
#pragma nounroll
        for (int l = 1; l < g.nc - 1; ++l) {
            if (TRAIN && crow) crow += gs.nsp * HD;
            layer<PREC, KS, T, true, OUT_B, 0, true>(st, c, nxt, nullptr, b, lane, crow, HD);
            b += 32 * T;
#pragma unroll
            for (int j = 0; j < KS; ++j) c[j] = nxt[j];
        }
        color_head(c, b);
    }
    if (h == 0 && valid) {
        f32x4 o;
        o[0] = sig[0];
#pragma unroll
        for (int k = 0; k < 3; ++k) o[1 + k] = 1.f / (1.f + expf(-col[k]));      // torch.sigmoid(h) voxnerf.py:252
        *reinterpret_cast<f32x4*>(p.raw + s * 4) = o;
    }
}

template <int PREC, int HD, bool S1, bool C1, bool TRAIN = false>
static int launch_gen(const VoxMlpParams& p, const VoxGenShape& g, hipStream_t st) {
    constexpr int NT = mlp_threads(PREC);
    const long blocks = cdiv(p.nsamp, NT / 2);
    const size_t lds = MlpLds<PREC>::TOTAL;
    EVD_SET_MAX_LDS((&k_voxel_mlp_generic<PREC, HD, S1, C1, TRAIN>), lds);
    hipLaunchKernelGGL((k_voxel_mlp_generic<PREC, HD, S1, C1, TRAIN>), dim3((unsigned)blocks), dim3(NT), lds, st, p, g);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

static int gen_shape_check(const VoxMlpParams& p, const VoxGenShape& g) {
    if (g.ns < 1 || g.ns > VG_MAX_LAYERS || g.nc < 1 || g.nc > VG_MAX_LAYERS || g.gt < 1 || g.gt > VG_GT || g.G < 1 || g.G > 32 * g.gt ||
        g.kf < 1 || g.kf > VG_KF || p.ft_stride < 16 * g.kf || p.nbias > MlpLds<EVD_PREC_F32>::BIAS_FLOATS)
        return fail(EVD_E_INVALID, "evd_voxel: generic level shape out of range (layers %d + %d, geo %d in %d tiles, %d feature k-steps, row stride %d)",
                    g.ns, g.nc, g.G, g.gt, g.kf, p.ft_stride);
    return EVD_OK;
}

int voxel_train_fwd_generic_dispatch(int HD, const VoxMlpParams& p, const VoxGenShape& g, hipStream_t st) {
    if (int rc = gen_shape_check(p, g)) return rc;
    if (!p.act) return fail(EVD_E_INVALID, "evd_voxel_mlp_train: no store");
#define EVD_CASE(H_)                                                                                                                            \
    if (HD == H_)                                                                                                                               \
        return g.ns == 1 ? (g.nc == 1 ? launch_gen<EVD_PREC_F16X3, H_, true, true, true>(p, g, st) : launch_gen<EVD_PREC_F16X3, H_, true, false, true>(p, g, st)) \
                         : (g.nc == 1 ? launch_gen<EVD_PREC_F16X3, H_, false, true, true>(p, g, st) : launch_gen<EVD_PREC_F16X3, H_, false, false, true>(p, g, st))
    EVD_CASE(64);
    EVD_CASE(128);
    EVD_CASE(256);
#undef EVD_CASE
    return fail(EVD_E_INVALID, "evd_voxel_mlp_train: no generic training kernel for hidden %d (built: 64, 128, 256)", HD);
}

int voxel_mlp_generic_dispatch(int prec, int HD, const VoxMlpParams& p, const VoxGenShape& g, hipStream_t st) {
    if (int rc = gen_shape_check(p, g)) return rc;
#define EVD_CASE(P, H_)                                                                                               \
    if (prec == P && HD == H_)                                                                                        \
        return g.ns == 1 ? (g.nc == 1 ? launch_gen<P, H_, true, true>(p, g, st) : launch_gen<P, H_, true, false>(p, g, st)) \
                         : (g.nc == 1 ? launch_gen<P, H_, false, true>(p, g, st) : launch_gen<P, H_, false, false>(p, g, st))
    EVD_CASE(EVD_PREC_BF16, 64);
    EVD_CASE(EVD_PREC_F16, 64);
    EVD_CASE(EVD_PREC_F16X3, 64);
    EVD_CASE(EVD_PREC_F32, 64);
    EVD_CASE(EVD_PREC_BF16, 128);
    EVD_CASE(EVD_PREC_F16, 128);
    EVD_CASE(EVD_PREC_F16X3, 128);
    EVD_CASE(EVD_PREC_F32, 128);
    EVD_CASE(EVD_PREC_BF16, 256);
    EVD_CASE(EVD_PREC_F16, 256);
    EVD_CASE(EVD_PREC_F16X3, 256);
    EVD_CASE(EVD_PREC_F32, 256);
#undef EVD_CASE
    return fail(EVD_E_INVALID, "evd_voxel: no generic level kernel for precision %d, hidden %d (built: hidden 64, 128, 256)", prec, HD);
}

}  // namespace evd
