// field_mlp.hip - fused radiance-field MLP forward for gfx950 (MI355X).
//
// What it replaces: the `network(inputs[M,6]) -> [M,4]` call inside run_network
// (reference nerf/render.py:59-75) for NeRF / SirenNeRF (nerf/nerf.py:52-170), FilmSirenNeRF
// (pi_GAN/modules.py:70-118) and the build-defined TinyNeRF, including positional encoding
// (nerf/nerf.py:44-49), every Dense/Siren/FiLM layer, the sigma/rgb heads and - in ray mode -
// the point generation pts = o + d*z, view = d/|d| of render_rays (render.py:122,134).
//
// Structure (one workgroup = 4 waves = 128 points, one wave per SIMD, whole register file):
//   * features on MFMA rows, points on MFMA columns (v_mfma_f32_32x32x2_f32, exact fp32), so
//     the 8x16 accumulator registers of a 256-wide layer ARE the next layer's B operands:
//     activations never leave registers between layers;
//   * weights stream HBM/L2 -> LDS by global_load_lds_dwordx4 (1 KiB pieces) in the order the
//     MFMAs consume them (field_layout.h), double-buffered per 32-wide K block (32 KiB), one
//     barrier per K block; A fragments are ds_read_b128 (4 MFMAs per read);
//   * bias / head weights / K=3 input columns ride the same stream as 1 KiB VEC pieces into a
//     per-layer LDS aux slot; FiLM gamma|beta rows are DMA'd per image into a film slot;
//   * sigma / rgb heads (1 and 3 outputs) are VALU dot products + one cross-half shuffle.
// Roofline: fp32 MFMA (157 TFLOP/s); HBM traffic is 24-28 B in + 16 B out per point.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "field_kinds.h"
#include "field_mlp_device.h"

namespace mi {

// =========================================================================================
// NeRF (nerf/nerf.py:75-94) and TinyNeRF
// =========================================================================================
// SAVE = training forward: every linear layer's input is also written to HBM ([point][feature] rows,
// region table nerf_acts()/tiny_acts() in field_layout.h) for the backward pass.
// SIGMA_ONLY = density forward: the trunk and the sigma head, then the wave ends (store_sigma).  Up to sigma it executes
// the inference instance's instructions, so sigma has the same bits.
// WINDOW = the sigma-only instance over one window of samples of the live rays (load_window_point): a block whose tile lies
// past the live count returns before it issues any LDS DMA.
// SPILL = the trunk-and-spill instance of the fine pass's deferred colour branch: the sigma-only instance with another
// ending.  It writes {0, 0, 0, sigma} to out [M][4] and appends every point with sigma > 0 - its H8 row and its index - to
// the live list a.defer (spill_live); nerf_colour_kernel below then runs the colour branch over that list alone.  Only this
// instance's argument block carries the list: every other instance takes MlpArgs as before.
struct DeferMlpArgs : MlpArgs { DeferArgs defer; };
template <bool TINY, bool SAVE, bool SIGMA_ONLY, bool WINDOW = false, bool SPILL = false>
__global__ __launch_bounds__(256, 1) void nerf_fwd_kernel(std::conditional_t<SPILL, DeferMlpArgs, MlpArgs> a) {
    static_assert(!(SAVE && SIGMA_ONLY), "the training forward needs the colour branch");
    static_assert(!WINDOW || SIGMA_ONLY, "windows exist for the sigma-only coarse pass");
    static_assert(!SPILL || (SIGMA_ONLY && !WINDOW), "the spill is an ending of the sigma-only instance");
    constexpr FieldKind K = kFieldKinds[TINY ? MI_FIELD_TINY_NERF : MI_FIELD_NERF];
    // the stage the last trunk layer issues behind it: the colour branch's first, none if the wave stops at sigma
    constexpr int kNextAux = SIGMA_ONLY ? 0 : K.branch_aux_pieces();
    constexpr int kNextBlock = SIGMA_ONLY ? 0 : K.branch_block_pieces();
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int64_t group = WINDOW ? 0 : blockIdx.x / a.tiles_per_group;
    const int64_t tile = WINDOW ? blockIdx.x : blockIdx.x % a.tiles_per_group;
    int64_t live = 0;
    if constexpr (WINDOW) {
        live = window_live_count(a);
        if (tile * (128 >> a.win_log2) >= live) return;
    }
    Ctx c = make_ctx(smem, a, group);
    MI_STAMP(a, 0);
    issue_first_stage<1, 32, false>(c, 0);   // layer 0: bias + K block 0 (PE features 0..31)

    PointIn pt;
    if constexpr (WINDOW) pt = load_window_point(a, tile, live, c.wave * 32 + (c.lane & 31));
    else pt = load_point(a.mode, a.a, a.z, group, a.points_per_group, a.rays_per_group, a.n_samples,
                         tile * 128 + c.wave * 32 + (c.lane & 31));
    f32x16 pe[2], pd[1], X[8], acc[8];
    posenc_blocks<2>(c.h, pt.px, pt.py, pt.pz, 60, pe);
    posenc_blocks<1>(c.h, pt.dx, pt.dy, pt.dz, 24, pd);

    constexpr RegionLayout RL = TINY ? tiny_acts() : nerf_acts();
    const int64_t SP = a.save_points;
    // `sw`: the region of the layer's ReLU switch bits (nerf_acts() 12.. / tiny_acts() 7..), -1 for none
    const auto rows = [&](int off_floats_per_point, int width, int sw = -1) {
        return SaveRows{SAVE ? a.save + (int64_t)off_floats_per_point * SP : nullptr, width, pt.p, pt.valid,
                        SAVE && sw >= 0 ? a.save + (int64_t)region_offset(RL, sw) * SP : nullptr};
    };
    constexpr int SW0 = TINY ? 7 : 12;                     // switch region of H1; H_l: SW0 + l - 1; H_d: the last region
    if constexpr (SAVE) {
        f32x16 tmp[8];
        tmp[0] = pe[0]; tmp[1] = pe[1];
        store_rows<2>(a.save, 64, pt.p, pt.valid, c.h, tmp);
        tmp[0] = pd[0];
        store_rows<1>(a.save + (int64_t)region_offset(RL, TINY ? 5 : 10) * SP, 32, pt.p, pt.valid, c.h, tmp);
    }

    const auto sel_pe = [&](auto kb) -> const f32x16& { return pe[decltype(kb)::value]; };
    const auto sel_x = [&](auto kb) -> const f32x16& { return X[decltype(kb)::value]; };
    const auto sel_skip = [&](auto kb) -> const f32x16& {
        constexpr int k = decltype(kb)::value;
        if constexpr (k < 2) return pe[k]; else return X[k - 2];
    };
    const auto sel_dir = [&](auto kb) -> const f32x16& {
        constexpr int k = decltype(kb)::value;
        if constexpr (k < 8) return X[k]; else return pd[0];
    };

    int slot = 0;
    MI_STAMP(a, 1);
    // layers_pos[0]: 60 -> 256
    fwd_layer<2, 8, false, 1, 32, false, ACT_RELU, SAVE, true>(c, slot, 0, 0, 0.f, 0.f, 0.f, sel_pe, acc, X, nullptr, rows(64, 256, SW0));
    slot ^= 1;                                                          // H1
    MI_STAMP(a, 3);
    float sigma;
    if constexpr (!TINY) {
        // layers_pos[1..4]
#pragma unroll 1
        for (int l = 1; l <= 4; ++l) {
#ifdef MI_PROFILE_STAMPS
            if (l == 2 && a.stamps) c.rowst = a.stamps + (int64_t)blockIdx.x * 128 + 32;   // rows of layers_pos[2]: 32..64
#endif
            fwd_layer<8, 8, false, 1, 32, false, ACT_RELU, SAVE, true, 8>(c, slot, 0, 0, 0.f, 0.f, 0.f, sel_x, acc, X, nullptr,
                                                                          rows(64 + 256 * l, 256, SW0 + l), rows(64 + 256 * (l - 1), 256));   // H2..H5
            slot ^= 1;
            MI_ROW_STAMP(c);
#ifdef MI_PROFILE_STAMPS
            c.rowst = nullptr;
#endif
            MI_STAMP(a, 3 + 2 * l);
        }
        // layers_pos[5]: [PE(60) | h(256)] -> 256
        fwd_layer<10, 8, false, 1, 32, false, ACT_RELU, SAVE, true, 8>(c, slot, 0, 0, 0.f, 0.f, 0.f, sel_skip, acc, X, nullptr,
                                                                       rows(region_offset(RL, 6), 256, SW0 + 5), rows(region_offset(RL, 5), 256));   // H6
        slot ^= 1;
        MI_STAMP(a, 13);
        // layers_pos[6]
        fwd_layer<8, 8, false, 3, 32, false, ACT_RELU, SAVE, true, 8>(c, slot, 0, 0, 0.f, 0.f, 0.f, sel_x, acc, X, nullptr,
                                                                      rows(region_offset(RL, 7), 256, SW0 + 6), rows(region_offset(RL, 6), 256));    // H7
        slot ^= 1;
        MI_STAMP(a, 15);
        // layers_pos[7] (+ sigma head pieces)
        fwd_layer<8, 8, false, kNextAux, kNextBlock, false, ACT_RELU, SAVE, true, 8>(c, slot, 0, 0, 0.f, 0.f, 0.f, sel_x, acc, X, nullptr,
                                                                      rows(region_offset(RL, 8), 256, SW0 + 7), rows(region_offset(RL, 7), 256));    // H8
        sigma = sigma_head(X, smem + kLdsAux0 + slot * kLdsAux, c.h);
        slot ^= 1;
        MI_STAMP(a, 17);
        if constexpr (!SIGMA_ONLY) {
            // layers_dir[0]: linear
            fwd_layer<8, 8, false, 5, 16, false, ACT_LINEAR, SAVE, true, 8>(c, slot, 0, 0, 0.f, 0.f, 0.f, sel_x, acc, X, nullptr,
                                                                            rows(region_offset(RL, 9), 256), rows(region_offset(RL, 8), 256));  // G
            slot ^= 1;
            MI_STAMP(a, 19);
        }
    } else {
        // layers_pos[1], [2], [3] (+ sigma head pieces), then the dir layer's 5 aux pieces
        fwd_layer<8, 8, false, 1, 32, false, ACT_RELU, SAVE, true, 8>(c, slot, 0, 0, 0.f, 0.f, 0.f, sel_x, acc, X, nullptr,
                                                                      rows(region_offset(RL, 2), 256, SW0 + 1), rows(region_offset(RL, 1), 256));
        slot ^= 1;
        fwd_layer<8, 8, false, 3, 32, false, ACT_RELU, SAVE, true, 8>(c, slot, 0, 0, 0.f, 0.f, 0.f, sel_x, acc, X, nullptr,
                                                                      rows(region_offset(RL, 3), 256, SW0 + 2), rows(region_offset(RL, 2), 256));
        slot ^= 1;
        fwd_layer<8, 8, false, kNextAux, kNextBlock, false, ACT_RELU, SAVE, true, 8>(c, slot, 0, 0, 0.f, 0.f, 0.f, sel_x, acc, X, nullptr,
                                                                      rows(region_offset(RL, 4), 256, SW0 + 3), rows(region_offset(RL, 3), 256));
        sigma = sigma_head(X, smem + kLdsAux0 + slot * kLdsAux, c.h);
        slot ^= 1;
    }
    if constexpr (SPILL) {
        store_out(a, pt, c.h, 0.f, 0.f, 0.f, sigma);
        spill_live(a.defer, pt, c.lane, c.h, sigma, X);
        return;
    } else if constexpr (SIGMA_ONLY) {
        store_sigma(a, pt, c.h, sigma);
        return;
    }
    // layers_dir[1] (TinyNeRF: layers_dir[0]): [h(256) | PE_dir(24)] -> 128, relu; then rgb head
    fwd_layer<9, 4, false, 0, 0, false, ACT_RELU, SAVE, false, 8>(c, slot, 0, 0, 0.f, 0.f, 0.f, sel_dir, acc, X, nullptr,
                                                                  rows(region_offset(RL, TINY ? 6 : 11), 128, RL.n - 1),
                                                                  rows(region_offset(RL, TINY ? 4 : 9), 256));   // H_d; G / H4 from X
    MI_STAMP(a, 20);
    const float* aux = smem + kLdsAux0 + slot * kLdsAux;
    const float r = sigmoidf(head_dot<4>(X, aux, 1, c.h) + aux[4 * kPiece + 0]);
    const float g = sigmoidf(head_dot<4>(X, aux, 2, c.h) + aux[4 * kPiece + 1]);
    const float b = sigmoidf(head_dot<4>(X, aux, 3, c.h) + aux[4 * kPiece + 2]);
    store_out(a, pt, c.h, r, g, b, sigma);
    MI_STAMP(a, 21);
}

// The colour branch alone, over the live list a trunk-and-spill launch left (same `a`): one tile = 128 list entries, one wave
// per 32.  A point's H8 comes back from its row (load_rows), its view direction from its ray with load_point's expressions;
// the packed stream is entered at the colour branch's first stage (field_kinds.h: branch_stream_floats), which this kernel
// issues itself where the inference instance's last trunk layer issues it.  From there it runs that instance's fwd_layer
// instantiations and heads, so r, g, b have its bits; they go to out[idx], where sigma already is.  Grid-stride over the
// tiles below the device count: a frame's worst-case tiles would be several hundred thousand blocks that only read the count.
template <bool TINY>
__global__ __launch_bounds__(256, 1) void nerf_colour_kernel(DeferMlpArgs a) {
    const DeferArgs& d = a.defer;
    constexpr FieldKind K = kFieldKinds[TINY ? MI_FIELD_TINY_NERF : MI_FIELD_NERF];
    constexpr int kBranchAux = K.branch_aux_pieces(), kBranchBlock = K.branch_block_pieces();
    constexpr int kBranchBytes = K.branch_stream_floats() * (int)sizeof(float);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int64_t count = __builtin_amdgcn_readfirstlane(__hip_atomic_load(d.count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    Ctx c = make_ctx(smem, a, 0);
    const SaveRows none{nullptr, 0, 0, false};
    bool again = false;
    for (int64_t tile = blockIdx.x; tile * 128 < count; tile += gridDim.x) {
        if (again) __syncthreads();              // every wave has read the last tile's heads: the LDS may be refilled
        again = true;
        c.soff = kBranchBytes;
        c.buf = 0;
        issue_first_stage<kBranchAux, kBranchBlock, false>(c, 0);

        const int64_t entry = tile * 128 + c.wave * 32 + (c.lane & 31);
        const bool valid = entry < count;
        const int64_t ec = valid ? entry : count - 1;            // clamped like load_window_point's entries, masked on the store
        const int p = d.idx[ec];
        const float* r6 = a.a + (int64_t)(p / a.n_samples) * 6;
        const float d0 = r6[3], d1 = r6[4], d2 = r6[5];
        const float nrm = dir_norm(d0, d1, d2);
        f32x16 pd[1], X[8], acc[8];
        posenc_blocks<1>(c.h, d0 / nrm, d1 / nrm, d2 / nrm, 24, pd);
        load_rows<8>(d.rows, 256, ec, c.h, X);

        const auto sel_x = [&](auto kb) -> const f32x16& { return X[decltype(kb)::value]; };
        const auto sel_dir = [&](auto kb) -> const f32x16& {
            constexpr int k = decltype(kb)::value;
            if constexpr (k < 8) return X[k]; else return pd[0];
        };
        int slot = 0;
        if constexpr (!TINY) {
            fwd_layer<8, 8, false, 5, 16, false, ACT_LINEAR, false, true, 8>(c, slot, 0, 0, 0.f, 0.f, 0.f, sel_x, acc, X, nullptr, none, none);  // G
            slot ^= 1;
        }
        fwd_layer<9, 4, false, 0, 0, false, ACT_RELU, false, false, 8>(c, slot, 0, 0, 0.f, 0.f, 0.f, sel_dir, acc, X, nullptr, none, none);   // H_d
        const float* aux = smem + kLdsAux0 + slot * kLdsAux;
        const float r = sigmoidf(head_dot<4>(X, aux, 1, c.h) + aux[4 * kPiece + 0]);
        const float g = sigmoidf(head_dot<4>(X, aux, 2, c.h) + aux[4 * kPiece + 1]);
        const float b = sigmoidf(head_dot<4>(X, aux, 3, c.h) + aux[4 * kPiece + 2]);
        if (valid && c.h == 0) {
            float* o = a.out + (int64_t)p * 4;
            o[0] = r; o[1] = g; o[2] = b;
        }
    }
}

// =========================================================================================
// SirenNeRF (nerf/nerf.py:153-170): sin(30 * linear) layers on raw xyz / dir
// =========================================================================================
template <bool SAVE, bool SIGMA_ONLY, bool WINDOW = false>
__global__ __launch_bounds__(256, 1) void siren_fwd_kernel(MlpArgs a) {
    static_assert(!(SAVE && SIGMA_ONLY), "the training forward needs the colour branch");
    static_assert(!WINDOW || SIGMA_ONLY, "windows exist for the sigma-only coarse pass");
    constexpr FieldKind K = kFieldKinds[MI_FIELD_SIREN_NERF];
    constexpr int kNextAux = SIGMA_ONLY ? 0 : K.branch_aux_pieces();      // as in nerf_fwd_kernel
    constexpr int kNextBlock = SIGMA_ONLY ? 0 : K.branch_block_pieces();
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int64_t group = WINDOW ? 0 : blockIdx.x / a.tiles_per_group;
    const int64_t tile = WINDOW ? blockIdx.x : blockIdx.x % a.tiles_per_group;
    int64_t live = 0;
    if constexpr (WINDOW) {                        // as in nerf_fwd_kernel
        live = window_live_count(a);
        if (tile * (128 >> a.win_log2) >= live) return;
    }
    Ctx c = make_ctx(smem, a, group);
    issue_first_stage<4, 0, false>(c, 0);   // layers_pos[0]: bias + 3 weight columns (K = 3, VALU)

    PointIn pt;
    if constexpr (WINDOW) pt = load_window_point(a, tile, live, c.wave * 32 + (c.lane & 31));
    else pt = load_point(a.mode, a.a, a.z, group, a.points_per_group, a.rays_per_group, a.n_samples,
                         tile * 128 + c.wave * 32 + (c.lane & 31));
    f32x16 X[8], acc[8];
    const auto sel_x = [&](auto kb) -> const f32x16& { return X[decltype(kb)::value]; };
    constexpr RegionLayout RL = siren_acts();
    const int64_t SP = a.save_points;
    const auto region = [&](int idx) { return a.save + (int64_t)region_offset(RL, idx) * SP; };
    // sin layer l (1..8): X_l (cosine sign in the lowest bit) -> region l
    const auto sin_rows = [&](int l) {
        return SaveRows{SAVE ? a.save + (int64_t)(8 + 256 * (l - 1)) * SP : nullptr, 256, pt.p, pt.valid};
    };
    const SaveRows none{nullptr, 0, 0, false};
    const auto sin_act = [&](int l) {
        if constexpr (SAVE)
            activate_train<8, ACT_SIN30>(acc, X, nullptr, c.h, smem + kLdsAux0, a.save + (int64_t)(8 + 256 * (l - 1)) * SP, 256,
                                         pt.p, pt.valid);
        else
            activate<8, ACT_SIN30>(acc, X, nullptr, c.h, smem + kLdsAux0);
    };
    if constexpr (SAVE) {
        if (pt.valid && c.h == 0) {
            f32x4* xin = reinterpret_cast<f32x4*>(a.save + pt.p * 8);
            xin[0] = f32x4{pt.px, pt.py, pt.pz, pt.dx};
            xin[1] = f32x4{pt.dy, pt.dz, 0.f, 0.f};
        }
    }

    int slot = 0;
    __syncthreads();
    issue_first_stage<1, 32, false>(c, 1);
    init_acc<8, true>(smem + kLdsAux0, c.h, 1, pt.px, pt.py, pt.pz, acc);
    sin_act(1); slot ^= 1;
    // sin layers store their own (encoded) rows from the activation hook: nothing is deferred to the next layer
#pragma unroll 1
    for (int l = 1; l <= 3; ++l) {
        fwd_layer<8, 8, false, 1, 32, false, ACT_SIN30, SAVE, false, 0>(c, slot, 0, 0, 0.f, 0.f, 0.f, sel_x, acc, X, nullptr, sin_rows(l + 1), none);
        slot ^= 1;
    }
    fwd_layer<8, 8, false, 4, 32, false, ACT_SIN30, SAVE, false, 0>(c, slot, 0, 0, 0.f, 0.f, 0.f, sel_x, acc, X, nullptr, sin_rows(5), none);  // layers_pos[4]
    slot ^= 1;
    fwd_layer<8, 8, true, 1, 32, false, ACT_SIN30, SAVE, false, 0>(c, slot, 0, 1, pt.px, pt.py, pt.pz, sel_x, acc, X, nullptr, sin_rows(6), none);  // [5]: [pos | h]
    slot ^= 1;
    fwd_layer<8, 8, false, 3, 32, false, ACT_SIN30, SAVE, false, 0>(c, slot, 0, 0, 0.f, 0.f, 0.f, sel_x, acc, X, nullptr, sin_rows(7), none);  // [6]
    slot ^= 1;
    fwd_layer<8, 8, false, kNextAux, kNextBlock, false, ACT_SIN30, SAVE, false, 0>(c, slot, 0, 0, 0.f, 0.f, 0.f, sel_x, acc, X, nullptr, sin_rows(8), none);  // [7] + sigma head
    const float sigma = sigma_head(X, smem + kLdsAux0 + slot * kLdsAux, c.h);
    if constexpr (SIGMA_ONLY) {
        store_sigma(a, pt, c.h, sigma);
        return;
    }
    slot ^= 1;
    const SaveRows g_rows{SAVE ? region(9) : nullptr, 256, pt.p, pt.valid};
    fwd_layer<8, 8, false, 8, 16, false, ACT_LINEAR, SAVE, true, 0>(c, slot, 0, 0, 0.f, 0.f, 0.f, sel_x, acc, X, nullptr, g_rows,
                                                                    none);  // layers_dir[0] linear: G (stored by the next layer)
    slot ^= 1;
    fwd_layer<8, 4, true, 0, 0, false, ACT_SIN30, SAVE, false, 8>(c, slot, 0, 1, pt.dx, pt.dy, pt.dz, sel_x, acc, X, nullptr,
                                                                  SaveRows{SAVE ? region(10) : nullptr, 128, pt.p, pt.valid},
                                                                  g_rows);  // layers_dir[1]: [h | dir]; G from X
    const float* aux = smem + kLdsAux0 + slot * kLdsAux;
    const float r = sigmoidf(head_dot<4>(X, aux, 4, c.h) + aux[7 * kPiece + 0]);
    const float g = sigmoidf(head_dot<4>(X, aux, 5, c.h) + aux[7 * kPiece + 1]);
    const float b = sigmoidf(head_dot<4>(X, aux, 6, c.h) + aux[7 * kPiece + 2]);
    store_out(a, pt, c.h, r, g, b, sigma);
}

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
    static_assert(film_body_floats(8, USE_DIR, false) ==
                  packed_body_floats(kFieldKinds[USE_DIR ? MI_FIELD_FILM_SIREN_NERF : MI_FIELD_FILM_SIREN_NERF_NODIR].fwd));
    const int kBody = film_body_floats(L, USE_DIR, false);
    c.w0 = a.packed[kBody];
    issue_first_stage<4, 0, true>(c, 0, 0);   // input_layer: bias + 3 columns, FiLM row 0

    const PointIn pt = load_point(a.mode, a.a, a.z, group, a.points_per_group, a.rays_per_group, a.n_samples,
                                  tile * 128 + c.wave * 32 + (c.lane & 31));
    f32x16 X[8], acc[8];
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
    if constexpr (SAVE) {
        if (pt.valid && c.h == 0) {
            f32x4* xin = reinterpret_cast<f32x4*>(a.save + pt.p * 8);
            xin[0] = f32x4{pt.px, pt.py, pt.pz, pt.dx};
            xin[1] = f32x4{pt.dy, pt.dz, 0.f, 0.f};
        }
    }

    int slot = 0;
    __syncthreads();
    issue_first_stage<1, 32, true>(c, 1, 1);
    init_acc<8, true>(smem + kLdsAux0, c.h, 1, pt.px, pt.py, pt.pz, acc);
    film_act(0, 0); slot ^= 1;
#pragma unroll 1
    for (int l = 1; l <= L - 3; ++l) {                                               // hidden_layers[0..L-4]
        fwd_layer<8, 8, false, 1, 32, true, ACT_FILM, SAVE, false, 0>(c, slot, l + 1, 0, 0.f, 0.f, 0.f, sel_x, acc, X, film_row(slot), film_rows(l), none);
        slot ^= 1;
    }
    fwd_layer<8, 8, false, 3, 32, true, ACT_FILM, SAVE, false, 0>(c, slot, L - 1, 0, 0.f, 0.f, 0.f, sel_x, acc, X, film_row(slot), film_rows(L - 2), none);  // hidden_layers[L-3]
    slot ^= 1;
    fwd_layer<8, 8, false, USE_DIR ? 8 : 5, 32, true, ACT_FILM, SAVE, false, 0>(c, slot, L, 0, 0.f, 0.f, 0.f, sel_x, acc, X, film_row(slot), film_rows(L - 1), none);  // hidden_layers[L-2]
    const float sigma = sigma_head(X, smem + kLdsAux0 + slot * kLdsAux, c.h);
    slot ^= 1;
    fwd_layer<8, 8, USE_DIR, 0, 0, false, ACT_FILM, SAVE, false, 0>(c, slot, 0, 1, pt.dx, pt.dy, pt.dz, sel_x, acc, X, film_row(slot), film_rows(L), none);   // hidden_layer_rgb
    const float* aux = smem + kLdsAux0 + slot * kLdsAux;
    constexpr int hp = USE_DIR ? 4 : 1;
    const float r = sigmoidf(head_dot<8>(X, aux, hp + 0, c.h) + aux[(hp + 3) * kPiece + 0]);
    const float g = sigmoidf(head_dot<8>(X, aux, hp + 1, c.h) + aux[(hp + 3) * kPiece + 1]);
    const float b = sigmoidf(head_dot<8>(X, aux, hp + 2, c.h) + aux[(hp + 3) * kPiece + 2]);
    store_out(a, pt, c.h, r, g, b, sigma);
}

// ---- host side ---------------------------------------------------------------------------
// [kind][variant]: the inference, the training (layer inputs saved), the sigma-only and the windowed sigma-only instance
// of each kind's kernel.
// The FiLM kinds have no sigma-only instance (their caller, pi_GAN, renders both passes with one field and needs the
// coarse colours for the merge): has_sigma_only_kernel() is false for them.
enum FwdVariant : int { FWD_INFER = 0, FWD_SAVE = 1, FWD_SIGMA = 2, FWD_SIGMA_WINDOW = 3 };
static const void* const kFwdKernels[MI_FIELD_KINDS][4] = {
    {(const void*)nerf_fwd_kernel<false, false, false>, (const void*)nerf_fwd_kernel<false, true, false>,
     (const void*)nerf_fwd_kernel<false, false, true>, (const void*)nerf_fwd_kernel<false, false, true, true>},   // MI_FIELD_NERF
    {(const void*)siren_fwd_kernel<false, false>, (const void*)siren_fwd_kernel<true, false>,
     (const void*)siren_fwd_kernel<false, true>, (const void*)siren_fwd_kernel<false, true, true>},           // MI_FIELD_SIREN_NERF
    {(const void*)film_fwd_kernel<true, false>, (const void*)film_fwd_kernel<true, true>, nullptr, nullptr},    // MI_FIELD_FILM_SIREN_NERF
    {(const void*)film_fwd_kernel<false, false>, (const void*)film_fwd_kernel<false, true>, nullptr, nullptr},  // ..._NODIR
    {(const void*)nerf_fwd_kernel<true, false, false>, (const void*)nerf_fwd_kernel<true, true, false>,
     (const void*)nerf_fwd_kernel<true, false, true>, (const void*)nerf_fwd_kernel<true, false, true, true>}};    // MI_FIELD_TINY_NERF

// [use_dir][variant]: the run-time-depth FiLM instances (MI_FIELD_FILM_DEPTH kinds other than depth 8, which IS kinds 2 / 3)
static const void* const kFilmDepthFwdKernels[2][2] = {
    {(const void*)film_fwd_kernel<false, false, true>, (const void*)film_fwd_kernel<false, true, true>},
    {(const void*)film_fwd_kernel<true, false, true>, (const void*)film_fwd_kernel<true, true, true>}};

// [kind]: the trunk-and-spill instance and the colour-branch kernel of the deferred colour branch (NeRF, TinyNeRF)
static const void* const kSpillKernels[MI_FIELD_KINDS] = {(const void*)nerf_fwd_kernel<false, false, true, false, true>, nullptr, nullptr,
                                                          nullptr, (const void*)nerf_fwd_kernel<true, false, true, false, true>};
static const void* const kColourKernels[MI_FIELD_KINDS] = {(const void*)nerf_colour_kernel<false>, nullptr, nullptr, nullptr,
                                                           (const void*)nerf_colour_kernel<true>};

bool has_deferred_colour_kernels(int kind) { return kind >= 0 && kind < MI_FIELD_KINDS && kSpillKernels[kind] && kColourKernels[kind]; }
bool has_sigma_only_kernel(int kind) { return kind >= 0 && kind < MI_FIELD_KINDS && kFwdKernels[kind][FWD_SIGMA]; }

// 148 KiB of dynamic LDS: raise the per-kernel limit once per device (host-side attribute, no device work)
static int raise_lds_limit(size_t lds) {
    static PerDeviceOnce attr_once;
    return attr_once.run([&]() {
        for (const auto& k : kFwdKernels)
            for (const void* f : k) {
                if (!f) continue;
                const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
                if (e != hipSuccess) { set_error("hipFuncSetAttribute: %s", hipGetErrorString(e)); return -2; }
            }
        for (const auto& k : kFilmDepthFwdKernels)
            for (const void* f : k) {
                const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
                if (e != hipSuccess) { set_error("hipFuncSetAttribute: %s", hipGetErrorString(e)); return -2; }
            }
        for (const auto* tab : {kSpillKernels, kColourKernels})
            for (int k = 0; k < MI_FIELD_KINDS; ++k) {
                if (!tab[k]) continue;
                const hipError_t e = hipFuncSetAttribute(tab[k], hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
                if (e != hipSuccess) { set_error("hipFuncSetAttribute: %s", hipGetErrorString(e)); return -2; }
            }
        return 0;
    });
}

int launch_mlp(int kind_in, const MlpArgs& a, int64_t n_groups, hipStream_t stream, bool sigma_only) {
    const int kind = canon_kind(kind_in);
    const int64_t blocks = n_groups * a.tiles_per_group;
    if (blocks <= 0) return 0;
    if (blocks > 0x7fffffffLL) { set_error("too many point tiles (%lld)", (long long)blocks); return -1; }
    if (bad_kind(kind)) return -1;
    if (sigma_only && (a.save || !has_sigma_only_kernel(kind))) {
        set_error("kind %d has no sigma-only forward%s", kind, a.save ? " with saved layer inputs" : "");
        return -1;
    }
    const size_t lds = kLdsFloats * sizeof(float);
    if (const int arc = raise_lds_limit(lds)) return arc;
    void* args[] = {const_cast<MlpArgs*>(&a)};
    const int variant = sigma_only ? FWD_SIGMA : a.save ? FWD_SAVE : FWD_INFER;
    const void* fn;
    if (is_depth_kind(kind)) {
        if (a.film_depth != film_depth(kind) || !a.film) { set_error("FiLM depth kind 0x%x launched without its depth or table", kind); return -1; }
        fn = kFilmDepthFwdKernels[film_use_dir(kind)][variant];
    } else {
        fn = kFwdKernels[kind][variant];
    }
    (void)hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(256), args, lds, stream);
    return check_launch("field_mlp_fwd");
}

int launch_mlp_window(int kind_in, const MlpArgs& a, hipStream_t stream) {
    const int kind = canon_kind(kind_in);
    if (bad_kind(kind)) return -1;
    if (a.save || a.film || !has_sigma_only_kernel(kind) || a.win_log2 < 0 || a.win_log2 > 7 || a.win_k0 < 0 ||
        a.win_k0 >= a.n_samples || a.n_rays > 0x7fffffffLL) {
        set_error("kind %d: bad windowed sigma-only launch", kind);
        return -1;
    }
    const int64_t per_tile = 128 >> a.win_log2;
    const int64_t blocks = (a.n_rays + per_tile - 1) / per_tile;        // worst case: every ray live
    if (blocks <= 0) return 0;
    if (blocks > 0x7fffffffLL) { set_error("too many point tiles (%lld)", (long long)blocks); return -1; }
    const size_t lds = kLdsFloats * sizeof(float);
    if (const int arc = raise_lds_limit(lds)) return arc;
    void* args[] = {const_cast<MlpArgs*>(&a)};
    (void)hipLaunchKernel(kFwdKernels[kind][FWD_SIGMA_WINDOW], dim3((unsigned)blocks), dim3(256), args, lds, stream);
    return check_launch("field_mlp_fwd_window");
}

// compute units of the current device, asked once per device ordinal (0 and the error set if the query fails)
static int compute_units() {
    static std::atomic<int> cached[256] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 256) { set_error("hipGetDevice failed"); return 0; }
    int cus = cached[dev].load(std::memory_order_relaxed);
    if (cus < 1) {
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) {
            set_error("field_mlp_colour: no compute-unit count");
            return 0;
        }
        cached[dev].store(cus, std::memory_order_relaxed);
    }
    return cus;
}

// shared checks of the two deferred-colour launches: a mode-1 launch of one group whose point indices fit the list's ints
static int check_deferred(int kind, const MlpArgs& a, const DeferArgs& d) {
    if (bad_kind(kind)) return -1;
    if (!has_deferred_colour_kernels(kind) || a.save || a.film || a.mode != 1 || a.n_samples < 1 || !d.rows || !d.idx || !d.count ||
        a.points_per_group < 1 || a.points_per_group > 0x7fffffffLL || a.tiles_per_group != (a.points_per_group + 127) / 128) {
        set_error("kind %d: bad deferred-colour launch", kind);
        return -1;
    }
    return raise_lds_limit(kLdsFloats * sizeof(float));
}

int launch_mlp_trunk_spill(int kind, const MlpArgs& a, const DeferArgs& d, hipStream_t stream) {
    if (const int rc = check_deferred(kind, a, d)) return rc;
    DeferMlpArgs da{a, d};
    void* args[] = {&da};
    (void)hipLaunchKernel(kSpillKernels[kind], dim3((unsigned)a.tiles_per_group), dim3(256), args, kLdsFloats * sizeof(float), stream);
    return check_launch("field_mlp_trunk_spill");
}

int launch_mlp_colour(int kind, const MlpArgs& a, const DeferArgs& d, hipStream_t stream) {
    if (const int rc = check_deferred(kind, a, d)) return rc;
    // one block per CU (148 KiB of LDS each) strides over the tiles below the device count; never more blocks than tiles
    const int cus = compute_units();
    if (cus < 1) return -2;
    const int64_t blocks = a.tiles_per_group < cus ? a.tiles_per_group : cus;
    DeferMlpArgs da{a, d};
    void* args[] = {&da};
    (void)hipLaunchKernel(kColourKernels[kind], dim3((unsigned)blocks), dim3(256), args, kLdsFloats * sizeof(float), stream);
    return check_launch("field_mlp_colour");
}

}  // namespace mi
