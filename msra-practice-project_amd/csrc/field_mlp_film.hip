// field_mlp_film.hip - the FilmSirenNeRF kernel of the fused field-MLP forward (design: field_mlp.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "field_kinds.h"
#include "field_mlp_device.h"
#include "field_mlp_instances.h"

namespace mi {

// =========================================================================================
// FilmSirenNeRF (pi_GAN/modules.py:101-118): sin(30 * (gamma * linear + beta)), one FiLM
// table per group (image)
// =========================================================================================
// RT_DEPTH: hidden_layers = L is a run-time, wave-uniform value (MlpArgs::film_depth, 4..12: the MI_FIELD_FILM_DEPTH kinds)
// instead of the literal 8 of kinds 2 / 3, whose instances stay compile-time: one more instance per (USE_DIR, SAVE) serves
// every depth.  The stream has L - 2 plain hidden layers in the loop, then the two that prefetch the heads' pieces; FiLM
// layer l saves to region 1 + l; the trailer sits behind a body whose length follows L (so L cannot travel in it).
template <bool USE_DIR, bool SAVE, bool RT_DEPTH = false>
__global__ __launch_bounds__(256, 1) void film_fwd_kernel(MlpArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int64_t group = blockIdx.x / a.tiles_per_group;
    const int64_t tile = blockIdx.x % a.tiles_per_group;
    const int L = RT_DEPTH ? __builtin_amdgcn_readfirstlane(a.film_depth) : 8;
    Ctx c = make_ctx_raw(smem, a.packed, a.film + group * ((L + 1) * kFilmRow));
    // FilmSiren's w_0 (pi_GAN/modules.py:11,73): the first float of the stream's trailer, a uniform (scalar) load
    constexpr FieldKind K = kFieldKinds[USE_DIR ? MI_FIELD_FILM_SIREN_NERF : MI_FIELD_FILM_SIREN_NERF_NODIR];
    static_assert(film_body_floats(8, USE_DIR, false) == packed_body_floats(K.fwd));
    const int kBody = film_body_floats(L, USE_DIR, false);
    c.w0 = a.packed[kBody];
    // The shapes are depth 8's (kinds 2 / 3), by their distance from the stream's ends: segments 0 (input_layer, K = 3) and 1
    // from the front, N - 3 (the last plain hidden layer), N - 2 (the trunk's last, with the sigma head's pieces) and
    // N - 1 (hidden_layer_rgb, with the rgb head's) from the back, every one between like segment 1.  Any other depth's
    // stream has the same (field_kinds.h: film_depth_like_8).
    constexpr Segments F = segments(K.fwd);
    constexpr int N = F.n;
    static_assert(N == 8 + 1 && K.sigma_segments() == N - 1 && F.uniform(1, N - 4), "input_layer, the loop's hidden layers, two more, rgb hidden");
    static_assert(!RT_DEPTH || film_segments_ok(USE_DIR), "every depth's stream has depth 8's shapes at depth 8's distances from its ends");
    constexpr int kSigmaRow = F.seg[N - 2].piece(AUX_WROW, K.sigma_head), kSigmaBias = F.seg[N - 2].piece(AUX_SCALARS, K.sigma_head);
    constexpr int kRgbRow = F.seg[N - 1].piece(AUX_WROW, K.rgb_head()), kRgbBias = F.seg[N - 1].piece(AUX_SCALARS, K.rgb_head());
    static_assert(kSigmaRow >= 0 && kSigmaBias >= 0 && kRgbRow >= 0 && kRgbBias >= 0, "the heads' pieces ride with the layers in front of them");
    constexpr int kPosCols = F.seg[0].k3_piece(), kDirCols = F.seg[N - 1].k3_piece();
    static_assert(kPosCols >= 0 && (kDirCols >= 0) == USE_DIR, "the K = 3 columns: xyz, and the direction if it is read");
    constexpr int kXBlocks = 8;                                            // K blocks sel_x serves
    static_assert(F.blocks(0) == 0 && F.blocks(1) == kXBlocks && F.blocks(N - 3) == kXBlocks && F.blocks(N - 2) == kXBlocks &&
                      F.blocks(N - 1) == kXBlocks, "every MFMA layer's K blocks are X's");
    issue_first_stage<F.aux(0), F.block_pieces(0), true>(c, 0, 0);   // input_layer: bias + 3 columns, FiLM row 0

    const PointIn pt = load_point(a.mode, a.a, a.z, group, a.points_per_group, a.rays_per_group, a.n_samples,
                                  tile * 128 + c.wave * 32 + (c.lane & 31));
    f32x16 X[kXBlocks], acc[8];
    const auto sel_x = [&](auto kb) -> const f32x16& { return X[decltype(kb)::value]; };
    const auto film_row = [&](int s) { return smem + kLdsFilm0 + s * kFilmRow; };
    const int64_t SP = a.save_points;
    // FiLM layer l (0..L): X_l (cosine sign in the lowest bit) -> region 1+l (256 wide, after the 8-wide xin)
    const auto film_rows = [&](int l) {
        return SaveRows{SAVE ? a.save + (int64_t)(8 + 256 * l) * SP : nullptr, 256, pt.p, pt.valid};
    };
    const SaveRows none{nullptr, 0, 0, false};
    const auto film_act = [&](int l, int slot_) {
        if constexpr (SAVE)
            activate_train<8, ACT_FILM>(acc, X, film_row(slot_), c.h, smem + kLdsAux0, a.save + (int64_t)(8 + 256 * l) * SP, 256,
                                        pt.p, pt.valid, c.w0);
        else
            activate<8, ACT_FILM>(acc, X, film_row(slot_), c.h, smem + kLdsAux0, c.w0);
    };
    if constexpr (SAVE) store_xin(a.save, pt, pt.valid && c.h == 0);

    int slot = 0;
    __syncthreads();
    issue_first_stage<F.aux(1), F.block_pieces(1), true>(c, 1, 1);
    init_acc<8, true>(smem + kLdsAux0, c.h, kPosCols, pt.px, pt.py, pt.pz, acc);
    film_act(0, 0); slot ^= 1;
#pragma unroll 1
    for (int l = 1; l <= L - 3; ++l) {                                               // hidden_layers[0..L-4]
        fwd_layer<F.blocks(1), F.mb(1), false, F.aux(2), F.block_pieces(2), true, ACT_FILM, SAVE, false, 0>(
            c, slot, l + 1, 0, 0.f, 0.f, 0.f, sel_x, acc, X, film_row(slot), film_rows(l), none);
        slot ^= 1;
    }
    fwd_layer<F.blocks(N - 3), F.mb(N - 3), false, F.aux(N - 2), F.block_pieces(N - 2), true, ACT_FILM, SAVE, false, 0>(
        c, slot, L - 1, 0, 0.f, 0.f, 0.f, sel_x, acc, X, film_row(slot), film_rows(L - 2), none);  // hidden_layers[L-3]
    slot ^= 1;
    fwd_layer<F.blocks(N - 2), F.mb(N - 2), false, F.aux(N - 1), F.block_pieces(N - 1), true, ACT_FILM, SAVE, false, 0>(
        c, slot, L, 0, 0.f, 0.f, 0.f, sel_x, acc, X, film_row(slot), film_rows(L - 1), none);  // hidden_layers[L-2]
    const float sigma = sigma_head(X, smem + kLdsAux0 + slot * kLdsAux, kSigmaRow, kSigmaBias, c.h);
    slot ^= 1;
    // (without the direction the layer starts at zero and never reads its K = 3 piece)
    fwd_layer<F.blocks(N - 1), F.mb(N - 1), USE_DIR, F.aux(N), F.block_pieces(N), false, ACT_FILM, SAVE, false, 0>(
        c, slot, 0, kDirCols, pt.dx, pt.dy, pt.dz, sel_x, acc, X, film_row(slot), film_rows(L), none);   // hidden_layer_rgb
    float r, g, b;
    rgb_heads<F.mb(N - 1)>(X, smem + kLdsAux0 + slot * kLdsAux, kRgbRow, kRgbBias, c.h, r, g, b);
    store_out(a, pt, c.h, r, g, b, sigma);
}

// The rows of the forward's instance table (field_mlp_instances.h).  The FiLM kinds have no sigma-only instance (their
// caller, pi_GAN, renders both passes with one field and needs the coarse colours for the merge).
extern const void* const kFilmRows[4][FWD_VARIANTS] = {
    {(const void*)film_fwd_kernel<true, false>, (const void*)film_fwd_kernel<true, true>},                // MI_FIELD_FILM_SIREN_NERF
    {(const void*)film_fwd_kernel<false, false>, (const void*)film_fwd_kernel<false, true>},              // ..._NODIR
    {(const void*)film_fwd_kernel<false, false, true>, (const void*)film_fwd_kernel<false, true, true>},  // any depth, no dir
    {(const void*)film_fwd_kernel<true, false, true>, (const void*)film_fwd_kernel<true, true, true>}};   // any depth, dir

}  // namespace mi
