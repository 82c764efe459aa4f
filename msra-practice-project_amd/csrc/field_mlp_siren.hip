// field_mlp_siren.hip - the SirenNeRF kernel of the fused field-MLP forward (design: field_mlp.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "field_kinds.h"
#include "field_mlp_device.h"
#include "field_mlp_instances.h"

namespace mi {

// =========================================================================================
// SirenNeRF (nerf/nerf.py:153-170): sin(30 * linear) layers on raw xyz / dir
// =========================================================================================
template <bool SAVE, bool SIGMA_ONLY, bool WINDOW = false, bool LIST = false>
__global__ __launch_bounds__(256, 1) void siren_fwd_kernel(MlpArgs a) {
    static_assert(!(SAVE && SIGMA_ONLY), "the training forward needs the colour branch");
    static_assert(!WINDOW || SIGMA_ONLY, "windows exist for the sigma-only coarse pass");
    static_assert(!LIST || (!SIGMA_ONLY && !WINDOW), "the list drives the inference and the training instance");
    constexpr FieldKind K = kFieldKinds[MI_FIELD_SIREN_NERF];
    // forward segment i is layer i's, as in nerf_fwd_kernel; layer 0 is K = 3 (VALU): its segment has no K blocks
    constexpr Segments F = segments(K.fwd);
    constexpr int T = K.sigma_segments(), D = F.n - 1;
    static_assert(T == 8 && D == T + 1, "layers_pos[0..7], then layers_dir[0], [1]: the ten layers this kernel spells out");
    constexpr int kNextAux = SIGMA_ONLY ? 0 : F.aux(T);
    constexpr int kNextBlock = SIGMA_ONLY ? 0 : F.block_pieces(T);
    constexpr int kSigmaRow = F.seg[T - 1].piece(AUX_WROW, K.sigma_head), kSigmaBias = F.seg[T - 1].piece(AUX_SCALARS, K.sigma_head);
    constexpr int kRgbRow = F.seg[D].piece(AUX_WROW, K.rgb_head()), kRgbBias = F.seg[D].piece(AUX_SCALARS, K.rgb_head());
    static_assert(kSigmaRow >= 0 && kSigmaBias >= 0 && kRgbRow >= 0 && kRgbBias >= 0, "the heads' pieces ride with the layers in front of them");
    constexpr int kPosCols0 = F.seg[0].k3_piece(), kPosCols5 = F.seg[5].k3_piece(), kDirCols = F.seg[D].k3_piece();
    static_assert(kPosCols0 >= 0 && kPosCols5 >= 0 && kDirCols >= 0, "the K = 3 columns of layers_pos[0], the skip layer and layers_dir[1]");
    constexpr int kXBlocks = 8;                                            // K blocks sel_x serves
    static_assert(F.blocks(0) == 0 && F.uniform(1, 3) && F.blocks(1) == kXBlocks && F.blocks(4) == kXBlocks && F.blocks(5) == kXBlocks &&
                      F.blocks(6) == kXBlocks && F.blocks(7) == kXBlocks && F.blocks(8) == kXBlocks && F.blocks(9) == kXBlocks,
                  "the loop's segments have one shape, and every MFMA layer's K blocks are X's");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int64_t group = WINDOW || LIST ? 0 : blockIdx.x / a.tiles_per_group;
    const int64_t tile = WINDOW || LIST ? blockIdx.x : blockIdx.x % a.tiles_per_group;
    int64_t live = 0;
    if constexpr (WINDOW) {                        // as in nerf_fwd_kernel
        live = window_live_count(a);
        if (tile * (128 >> a.win_log2) >= live) return;
    }
    if constexpr (LIST) {
        live = window_live_count(a);
        if (tile * 128 >= live) return;
    }
    Ctx c = make_ctx(smem, a, group);
    issue_first_stage<F.aux(0), F.block_pieces(0), false>(c, 0);   // layers_pos[0]: bias + 3 weight columns (K = 3, VALU)

    PointIn pt;
    if constexpr (WINDOW) pt = load_window_point(a, tile, live, c.wave * 32 + (c.lane & 31));
    else if constexpr (LIST) pt = load_list_point(a, tile, live, c.wave * 32 + (c.lane & 31));
    else pt = load_point(a.mode, a.a, a.z, group, a.points_per_group, a.rays_per_group, a.n_samples,
                         tile * 128 + c.wave * 32 + (c.lane & 31));
    f32x16 X[kXBlocks], acc[8];
    const auto sel_x = [&](auto kb) -> const f32x16& { return X[decltype(kb)::value]; };
    constexpr RegionLayout RL = siren_acts();
    const int64_t SP = a.save_points;
    const int64_t srow = list_save_row<LIST && SAVE>(pt, tile, live, c.wave * 32 + (c.lane & 31));   // row of the saved regions
    const auto region = [&](int idx) { return a.save + (int64_t)region_offset(RL, idx) * SP; };
    // sin layer l (1..8): X_l (cosine sign in the lowest bit) -> region l
    const auto sin_rows = [&](int l) {
        return SaveRows{SAVE ? a.save + (int64_t)(8 + 256 * (l - 1)) * SP : nullptr, 256, srow, pt.valid};
    };
    const SaveRows none{nullptr, 0, 0, false};
    const auto sin_act = [&](int l) {
        if constexpr (SAVE)
            activate_train<8, ACT_SIN30>(acc, X, nullptr, c.h, smem + kLdsAux0, a.save + (int64_t)(8 + 256 * (l - 1)) * SP, 256,
                                         srow, pt.valid);
        else
            activate<8, ACT_SIN30>(acc, X, nullptr, c.h, smem + kLdsAux0);
    };
    if constexpr (SAVE && LIST) {
        PointIn at = pt;
        at.p = srow;
        store_xin(a.save, at, pt.valid && c.h == 0);
    } else if constexpr (SAVE) store_xin(a.save, pt, pt.valid && c.h == 0);

    int slot = 0;
    __syncthreads();
    issue_first_stage<F.aux(1), F.block_pieces(1), false>(c, 1);
    init_acc<8, true>(smem + kLdsAux0, c.h, kPosCols0, pt.px, pt.py, pt.pz, acc);
    sin_act(1); slot ^= 1;
    // sin layers store their own (encoded) rows from the activation hook: nothing is deferred to the next layer
#pragma unroll 1
    for (int l = 1; l <= 3; ++l) {
        fwd_layer<F.blocks(1), F.mb(1), false, F.aux(2), F.block_pieces(2), false, ACT_SIN30, SAVE, false, 0>(
            c, slot, 0, 0, 0.f, 0.f, 0.f, sel_x, acc, X, nullptr, sin_rows(l + 1), none);
        slot ^= 1;
    }
    fwd_layer<F.blocks(4), F.mb(4), false, F.aux(5), F.block_pieces(5), false, ACT_SIN30, SAVE, false, 0>(
        c, slot, 0, 0, 0.f, 0.f, 0.f, sel_x, acc, X, nullptr, sin_rows(5), none);  // layers_pos[4]
    slot ^= 1;
    fwd_layer<F.blocks(5), F.mb(5), true, F.aux(6), F.block_pieces(6), false, ACT_SIN30, SAVE, false, 0>(
        c, slot, 0, kPosCols5, pt.px, pt.py, pt.pz, sel_x, acc, X, nullptr, sin_rows(6), none);  // [5]: [pos | h]
    slot ^= 1;
    fwd_layer<F.blocks(6), F.mb(6), false, F.aux(7), F.block_pieces(7), false, ACT_SIN30, SAVE, false, 0>(
        c, slot, 0, 0, 0.f, 0.f, 0.f, sel_x, acc, X, nullptr, sin_rows(7), none);  // [6]
    slot ^= 1;
    fwd_layer<F.blocks(7), F.mb(7), false, kNextAux, kNextBlock, false, ACT_SIN30, SAVE, false, 0>(
        c, slot, 0, 0, 0.f, 0.f, 0.f, sel_x, acc, X, nullptr, sin_rows(8), none);  // [7] + sigma head
    const float sigma = sigma_head(X, smem + kLdsAux0 + slot * kLdsAux, kSigmaRow, kSigmaBias, c.h);
    if constexpr (SIGMA_ONLY) {
        store_sigma(a, pt, c.h, sigma);
        return;
    }
    slot ^= 1;
    const SaveRows g_rows{SAVE ? region(9) : nullptr, 256, srow, pt.valid};
    fwd_layer<F.blocks(8), F.mb(8), false, F.aux(9), F.block_pieces(9), false, ACT_LINEAR, SAVE, true, 0>(
        c, slot, 0, 0, 0.f, 0.f, 0.f, sel_x, acc, X, nullptr, g_rows, none);  // layers_dir[0] linear: G (stored by the next layer)
    slot ^= 1;
    fwd_layer<F.blocks(D), F.mb(D), true, F.aux(D + 1), F.block_pieces(D + 1), false, ACT_SIN30, SAVE, false, F.mb(8)>(
        c, slot, 0, kDirCols, pt.dx, pt.dy, pt.dz, sel_x, acc, X, nullptr, SaveRows{SAVE ? region(10) : nullptr, 128, srow, pt.valid},
        g_rows);  // layers_dir[1]: [h | dir]; G from X
    float r, g, b;
    rgb_heads<F.mb(D)>(X, smem + kLdsAux0 + slot * kLdsAux, kRgbRow, kRgbBias, c.h, r, g, b);
    store_out(a, pt, c.h, r, g, b, sigma);
}

// the row of the forward's instance table (field_mlp_instances.h): MI_FIELD_SIREN_NERF
extern const void* const kSirenRow[1][FWD_VARIANTS] = {
    {(const void*)siren_fwd_kernel<false, false>, (const void*)siren_fwd_kernel<true, false>, (const void*)siren_fwd_kernel<false, true>,
     (const void*)siren_fwd_kernel<false, true, true>, nullptr, nullptr, (const void*)siren_fwd_kernel<false, false, false, true>,
     (const void*)siren_fwd_kernel<true, false, false, true>}};

}  // namespace mi
