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
// LIST = the inference instance over a device-counted list of points (load_list_point: rendering with an occupancy grid): a
// block whose tile lies past the count returns before it issues any LDS DMA; behind the loader it is the inference instance.
// LIST + SAVE = the training instance over such a list: entry e evaluates point p = list[e], its raw row goes to out[p] and its
// saved rows (SaveRows, store_xin, the switch words) to row e of every region - compact, in list order (list_save_row).
struct DeferMlpArgs : MlpArgs { DeferArgs defer; };
template <bool TINY, bool SAVE, bool SIGMA_ONLY, bool WINDOW = false, bool SPILL = false, bool LIST = false>
__global__ __launch_bounds__(256, 1) void nerf_fwd_kernel(std::conditional_t<SPILL, DeferMlpArgs, MlpArgs> a) {
    static_assert(!(SAVE && SIGMA_ONLY), "the training forward needs the colour branch");
    static_assert(!WINDOW || SIGMA_ONLY, "windows exist for the sigma-only coarse pass");
    static_assert(!SPILL || (SIGMA_ONLY && !WINDOW), "the spill is an ending of the sigma-only instance");
    static_assert(!LIST || (!SIGMA_ONLY && !WINDOW && !SPILL), "the list drives the inference and the training instance");
    constexpr FieldKind K = kFieldKinds[TINY ? MI_FIELD_TINY_NERF : MI_FIELD_NERF];
    // Forward segment i is layer i's (field_layout.h): T - 1 the trunk's last, with the sigma head's pieces; D the dir layer,
    // with the rgb head's.  A layer issues, behind its own K blocks, the aux pieces and first K blocks of the segment after it.
    constexpr Segments F = segments(K.fwd);
    constexpr int T = K.sigma_segments(), D = F.n - 1;
    static_assert(T == K.trunk && T == (TINY ? 4 : 8) && D == (TINY ? T : T + 1), "the trunk layers this kernel spells out, one segment each, then layers_dir");
    // what the last trunk layer issues behind it: the colour branch's first segment, nothing if the wave stops at sigma
    constexpr int kNextAux = SIGMA_ONLY ? 0 : F.aux(T);
    constexpr int kNextBlock = SIGMA_ONLY ? 0 : F.block_pieces(T);
    constexpr int kSigmaRow = F.seg[T - 1].piece(AUX_WROW, K.sigma_head), kSigmaBias = F.seg[T - 1].piece(AUX_SCALARS, K.sigma_head);
    constexpr int kRgbRow = F.seg[D].piece(AUX_WROW, K.rgb_head()), kRgbBias = F.seg[D].piece(AUX_SCALARS, K.rgb_head());
    static_assert(kSigmaRow >= 0 && kSigmaBias >= 0 && kRgbRow >= 0 && kRgbBias >= 0, "the heads' pieces ride with the layers in front of them");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int64_t group = WINDOW || LIST ? 0 : blockIdx.x / a.tiles_per_group;
    const int64_t tile = WINDOW || LIST ? blockIdx.x : blockIdx.x % a.tiles_per_group;
    int64_t live = 0;
    if constexpr (WINDOW) {
        live = window_live_count(a);
        if (tile * (128 >> a.win_log2) >= live) return;
    }
    if constexpr (LIST) {
        live = window_live_count(a);
        if (tile * 128 >= live) return;
    }
    Ctx c = make_ctx(smem, a, group);
    MI_STAMP(a, 0);
    issue_first_stage<F.aux(0), F.block_pieces(0), false>(c, 0);   // layer 0: bias + K blocks 0, 1 (the PE features)

    PointIn pt;
    if constexpr (WINDOW) pt = load_window_point(a, tile, live, c.wave * 32 + (c.lane & 31));
    else if constexpr (LIST) pt = load_list_point(a, tile, live, c.wave * 32 + (c.lane & 31));
    else pt = load_point(a.mode, a.a, a.z, group, a.points_per_group, a.rays_per_group, a.n_samples,
                         tile * 128 + c.wave * 32 + (c.lane & 31));
    constexpr int kPeBlocks = 2, kDirBlocks = 1, kXBlocks = 8;      // K blocks the B-operand selectors below serve
    f32x16 pe[kPeBlocks], pd[kDirBlocks], X[kXBlocks], acc[8];
    posenc_blocks<2>(c.h, pt.px, pt.py, pt.pz, 60, pe);
    posenc_blocks<1>(c.h, pt.dx, pt.dy, pt.dz, 24, pd);

    constexpr RegionLayout RL = TINY ? tiny_acts() : nerf_acts();
    const int64_t SP = a.save_points;
    const int64_t srow = list_save_row<LIST && SAVE>(pt, tile, live, c.wave * 32 + (c.lane & 31));   // row of the saved regions
    // `sw`: the region of the layer's ReLU switch bits (nerf_acts() 12.. / tiny_acts() 7..), -1 for none
    const auto rows = [&](int off_floats_per_point, int width, int sw = -1) {
        return SaveRows{SAVE ? a.save + (int64_t)off_floats_per_point * SP : nullptr, width, srow, pt.valid,
                        SAVE && sw >= 0 ? a.save + (int64_t)region_offset(RL, sw) * SP : nullptr};
    };
    constexpr int SW0 = RL.relu_switch0();                 // switch region of H1; H_l: SW0 + l - 1; H_d: the last region
    if constexpr (SAVE) {
        f32x16 tmp[8];
        tmp[0] = pe[0]; tmp[1] = pe[1];
        store_rows<2>(a.save, 64, srow, pt.valid, c.h, tmp);
        tmp[0] = pd[0];
        store_rows<1>(a.save + (int64_t)region_offset(RL, TINY ? 5 : 10) * SP, 32, srow, pt.valid, c.h, tmp);
    }

    const auto sel_pe = [&](auto kb) -> const f32x16& { return pe[decltype(kb)::value]; };
    const auto sel_x = [&](auto kb) -> const f32x16& { return X[decltype(kb)::value]; };
    const auto sel_skip = [&](auto kb) -> const f32x16& {
        constexpr int k = decltype(kb)::value;
        if constexpr (k < kPeBlocks) return pe[k]; else return X[k - kPeBlocks];
    };
    const auto sel_dir = [&](auto kb) -> const f32x16& {
        constexpr int k = decltype(kb)::value;
        if constexpr (k < kXBlocks) return X[k]; else return pd[0];
    };
    // every segment's K blocks are what its layer's selector serves; a loop body's segments, and the ones behind them, have one shape
    static_assert(F.blocks(0) == kPeBlocks && F.blocks(D) == kXBlocks + kDirBlocks && F.uniform(1, TINY ? 1 : 4) &&
                      F.blocks(1) == kXBlocks && (TINY || F.blocks(5) == kPeBlocks + kXBlocks),
                  "layers 0, 1..4, the skip layer and the dir layer against their B operands");
    static_assert(F.blocks(T - 2) == kXBlocks && F.blocks(T - 1) == kXBlocks && (TINY || F.blocks(T) == kXBlocks),
                  "the layers between those against X");

    int slot = 0;
    MI_STAMP(a, 1);
    // layers_pos[0]: 60 -> 256
    fwd_layer<F.blocks(0), F.mb(0), false, F.aux(1), F.block_pieces(1), false, ACT_RELU, SAVE, true>(c, slot, 0, 0, 0.f, 0.f, 0.f, sel_pe, acc, X, nullptr,
                                                                                                      rows(64, 256, SW0));
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
            fwd_layer<F.blocks(1), F.mb(1), false, F.aux(2), F.block_pieces(2), false, ACT_RELU, SAVE, true, F.mb(0)>(
                c, slot, 0, 0, 0.f, 0.f, 0.f, sel_x, acc, X, nullptr, rows(64 + 256 * l, 256, SW0 + l), rows(64 + 256 * (l - 1), 256));   // H2..H5
            slot ^= 1;
            MI_ROW_STAMP(c);
#ifdef MI_PROFILE_STAMPS
            c.rowst = nullptr;
#endif
            MI_STAMP(a, 3 + 2 * l);
        }
        // layers_pos[5]: [PE(60) | h(256)] -> 256
        fwd_layer<F.blocks(5), F.mb(5), false, F.aux(6), F.block_pieces(6), false, ACT_RELU, SAVE, true, F.mb(4)>(
            c, slot, 0, 0, 0.f, 0.f, 0.f, sel_skip, acc, X, nullptr, rows(region_offset(RL, 6), 256, SW0 + 5), rows(region_offset(RL, 5), 256));   // H6
        slot ^= 1;
        MI_STAMP(a, 13);
        // layers_pos[6]
        fwd_layer<F.blocks(6), F.mb(6), false, F.aux(7), F.block_pieces(7), false, ACT_RELU, SAVE, true, F.mb(5)>(
            c, slot, 0, 0, 0.f, 0.f, 0.f, sel_x, acc, X, nullptr, rows(region_offset(RL, 7), 256, SW0 + 6), rows(region_offset(RL, 6), 256));    // H7
        slot ^= 1;
        MI_STAMP(a, 15);
        // layers_pos[7] (+ sigma head pieces)
        fwd_layer<F.blocks(7), F.mb(7), false, kNextAux, kNextBlock, false, ACT_RELU, SAVE, true, F.mb(6)>(
            c, slot, 0, 0, 0.f, 0.f, 0.f, sel_x, acc, X, nullptr, rows(region_offset(RL, 8), 256, SW0 + 7), rows(region_offset(RL, 7), 256));    // H8
        sigma = sigma_head(X, smem + kLdsAux0 + slot * kLdsAux, kSigmaRow, kSigmaBias, c.h);
        slot ^= 1;
        MI_STAMP(a, 17);
        if constexpr (!SIGMA_ONLY) {
            // layers_dir[0]: linear
            fwd_layer<F.blocks(8), F.mb(8), false, F.aux(9), F.block_pieces(9), false, ACT_LINEAR, SAVE, true, F.mb(7)>(
                c, slot, 0, 0, 0.f, 0.f, 0.f, sel_x, acc, X, nullptr, rows(region_offset(RL, 9), 256), rows(region_offset(RL, 8), 256));  // G
            slot ^= 1;
            MI_STAMP(a, 19);
        }
    } else {
        // layers_pos[1], [2], [3] (+ sigma head pieces), then the dir layer's aux pieces
        fwd_layer<F.blocks(1), F.mb(1), false, F.aux(2), F.block_pieces(2), false, ACT_RELU, SAVE, true, F.mb(0)>(
            c, slot, 0, 0, 0.f, 0.f, 0.f, sel_x, acc, X, nullptr, rows(region_offset(RL, 2), 256, SW0 + 1), rows(region_offset(RL, 1), 256));
        slot ^= 1;
        fwd_layer<F.blocks(2), F.mb(2), false, F.aux(3), F.block_pieces(3), false, ACT_RELU, SAVE, true, F.mb(1)>(
            c, slot, 0, 0, 0.f, 0.f, 0.f, sel_x, acc, X, nullptr, rows(region_offset(RL, 3), 256, SW0 + 2), rows(region_offset(RL, 2), 256));
        slot ^= 1;
        fwd_layer<F.blocks(3), F.mb(3), false, kNextAux, kNextBlock, false, ACT_RELU, SAVE, true, F.mb(2)>(
            c, slot, 0, 0, 0.f, 0.f, 0.f, sel_x, acc, X, nullptr, rows(region_offset(RL, 4), 256, SW0 + 3), rows(region_offset(RL, 3), 256));
        sigma = sigma_head(X, smem + kLdsAux0 + slot * kLdsAux, kSigmaRow, kSigmaBias, c.h);
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
    fwd_layer<F.blocks(D), F.mb(D), false, F.aux(D + 1), F.block_pieces(D + 1), false, ACT_RELU, SAVE, false, F.mb(D - 1)>(
        c, slot, 0, 0, 0.f, 0.f, 0.f, sel_dir, acc, X, nullptr, rows(region_offset(RL, TINY ? 6 : 11), 128, RL.n - 1),
        rows(region_offset(RL, TINY ? 4 : 9), 256));   // H_d; G / H4 from X
    MI_STAMP(a, 20);
    float r, g, b;
    rgb_heads<F.mb(D)>(X, smem + kLdsAux0 + slot * kLdsAux, kRgbRow, kRgbBias, c.h, r, g, b);
    store_out(a, pt, c.h, r, g, b, sigma);
    MI_STAMP(a, 21);
}

// The colour branch alone, over the live list a trunk-and-spill launch left (same `a`): one tile = 128 list entries, one wave
// per 32.  A point's H8 comes back from its row (load_rows), its view direction from its ray with load_point's expressions;
// the packed stream is entered at the colour branch's first segment (field_kinds.h: sigma_segments()), which this kernel
// issues itself where the inference instance's last trunk layer issues it.  From there it runs that instance's fwd_layer
// instantiations and heads, so r, g, b have its bits; they go to out[idx], where sigma already is.  Grid-stride over the
// tiles below the device count: a frame's worst-case tiles would be several hundred thousand blocks that only read the count.
template <bool TINY>
__global__ __launch_bounds__(256, 1) void nerf_colour_kernel(DeferMlpArgs a) {
    const DeferArgs& d = a.defer;
    constexpr FieldKind K = kFieldKinds[TINY ? MI_FIELD_TINY_NERF : MI_FIELD_NERF];
    constexpr Segments F = segments(K.fwd);                 // as in nerf_fwd_kernel: T the branch's first segment, D the dir layer's
    constexpr int T = K.sigma_segments(), D = F.n - 1;
    static_assert(D == (TINY ? T : T + 1), "the colour branch: layers_dir, the whole of the stream behind the trunk");
    constexpr int kBranchBytes = F.seg[T].off * (int)sizeof(float);
    constexpr int kRgbRow = F.seg[D].piece(AUX_WROW, K.rgb_head()), kRgbBias = F.seg[D].piece(AUX_SCALARS, K.rgb_head());
    static_assert(kRgbRow >= 0 && kRgbBias >= 0, "the rgb head's pieces ride with the dir layer");
    constexpr int kDirBlocks = 1, kXBlocks = 8;              // K blocks the B-operand selectors below serve
    static_assert(F.blocks(D) == kXBlocks + kDirBlocks && (TINY || F.blocks(T) == kXBlocks), "layers_dir against their B operands");
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
        issue_first_stage<F.aux(T), F.block_pieces(T), false>(c, 0);

        const int64_t entry = tile * 128 + c.wave * 32 + (c.lane & 31);
        const bool valid = entry < count;
        const int64_t ec = valid ? entry : count - 1;            // clamped like load_window_point's entries, masked on the store
        const int p = d.idx[ec];
        const float* r6 = a.a + (int64_t)(p / a.n_samples) * 6;
        const float d0 = r6[3], d1 = r6[4], d2 = r6[5];
        const float nrm = dir_norm(d0, d1, d2);
        f32x16 pd[kDirBlocks], X[kXBlocks], acc[8];
        posenc_blocks<1>(c.h, d0 / nrm, d1 / nrm, d2 / nrm, 24, pd);
        load_rows<8>(d.rows, 256, ec, c.h, X);

        const auto sel_x = [&](auto kb) -> const f32x16& { return X[decltype(kb)::value]; };
        const auto sel_dir = [&](auto kb) -> const f32x16& {
            constexpr int k = decltype(kb)::value;
            if constexpr (k < kXBlocks) return X[k]; else return pd[0];
        };
        int slot = 0;
        if constexpr (!TINY) {
            fwd_layer<F.blocks(T), F.mb(T), false, F.aux(D), F.block_pieces(D), false, ACT_LINEAR, false, true, F.mb(T - 1)>(
                c, slot, 0, 0, 0.f, 0.f, 0.f, sel_x, acc, X, nullptr, none, none);  // G
            slot ^= 1;
        }
        fwd_layer<F.blocks(D), F.mb(D), false, F.aux(D + 1), F.block_pieces(D + 1), false, ACT_RELU, false, false, F.mb(D - 1)>(
            c, slot, 0, 0, 0.f, 0.f, 0.f, sel_dir, acc, X, nullptr, none, none);   // H_d
        float r, g, b;
        rgb_heads<F.mb(D)>(X, smem + kLdsAux0 + slot * kLdsAux, kRgbRow, kRgbBias, c.h, r, g, b);
        if (valid && c.h == 0) {
            float* o = a.out + (int64_t)p * 4;
            o[0] = r; o[1] = g; o[2] = b;
        }
    }
}

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

// ---- host side ---------------------------------------------------------------------------
// One table of instances, [row][variant].  Rows: the fixed kinds, then the run-time-depth FiLM instances without / with the
// direction (MI_FIELD_FILM_DEPTH kinds other than depth 8, which IS kinds 2 / 3).  Variants: the inference, the training
// (layer inputs saved), the sigma-only and the windowed sigma-only instance of the kind's kernel, then the two kernels of the
// deferred colour branch (NeRF, TinyNeRF): the trunk-and-spill instance and the colour-branch kernel, then the list-driven
// inference instance and the list-driven training instance (NeRF, SirenNeRF, TinyNeRF: the kinds an occupancy grid exists for).
// The FiLM kinds have no sigma-only instance (their caller, pi_GAN, renders both passes with one field and needs the
// coarse colours for the merge): has_sigma_only_kernel() is false for them.
enum FwdVariant : int { FWD_INFER = 0, FWD_SAVE, FWD_SIGMA, FWD_SIGMA_WINDOW, FWD_SPILL, FWD_COLOUR, FWD_LIST, FWD_LIST_SAVE, FWD_VARIANTS };
constexpr int kFilmDepthRow = MI_FIELD_KINDS;      // + use_dir
static const void* const kKernels[MI_FIELD_KINDS + 2][FWD_VARIANTS] = {
    // MI_FIELD_NERF
    {(const void*)nerf_fwd_kernel<false, false, false>, (const void*)nerf_fwd_kernel<false, true, false>,
     (const void*)nerf_fwd_kernel<false, false, true>, (const void*)nerf_fwd_kernel<false, false, true, true>,
     (const void*)nerf_fwd_kernel<false, false, true, false, true>, (const void*)nerf_colour_kernel<false>,
     (const void*)nerf_fwd_kernel<false, false, false, false, false, true>,
     (const void*)nerf_fwd_kernel<false, true, false, false, false, true>},
    // MI_FIELD_SIREN_NERF
    {(const void*)siren_fwd_kernel<false, false>, (const void*)siren_fwd_kernel<true, false>, (const void*)siren_fwd_kernel<false, true>,
     (const void*)siren_fwd_kernel<false, true, true>, nullptr, nullptr, (const void*)siren_fwd_kernel<false, false, false, true>,
     (const void*)siren_fwd_kernel<true, false, false, true>},
    {(const void*)film_fwd_kernel<true, false>, (const void*)film_fwd_kernel<true, true>},                // MI_FIELD_FILM_SIREN_NERF
    {(const void*)film_fwd_kernel<false, false>, (const void*)film_fwd_kernel<false, true>},              // ..._NODIR
    // MI_FIELD_TINY_NERF
    {(const void*)nerf_fwd_kernel<true, false, false>, (const void*)nerf_fwd_kernel<true, true, false>,
     (const void*)nerf_fwd_kernel<true, false, true>, (const void*)nerf_fwd_kernel<true, false, true, true>,
     (const void*)nerf_fwd_kernel<true, false, true, false, true>, (const void*)nerf_colour_kernel<true>,
     (const void*)nerf_fwd_kernel<true, false, false, false, false, true>,
     (const void*)nerf_fwd_kernel<true, true, false, false, false, true>},
    {(const void*)film_fwd_kernel<false, false, true>, (const void*)film_fwd_kernel<false, true, true>},  // any depth, no dir
    {(const void*)film_fwd_kernel<true, false, true>, (const void*)film_fwd_kernel<true, true, true>}};   // any depth, dir

bool has_deferred_colour_kernels(int kind) { return kind >= 0 && kind < MI_FIELD_KINDS && kKernels[kind][FWD_SPILL] && kKernels[kind][FWD_COLOUR]; }
bool has_sigma_only_kernel(int kind) { return kind >= 0 && kind < MI_FIELD_KINDS && kKernels[kind][FWD_SIGMA]; }
bool has_list_kernel(int kind) { return kind >= 0 && kind < MI_FIELD_KINDS && kKernels[kind][FWD_LIST] && kKernels[kind][FWD_LIST_SAVE]; }

// Every instance runs 256 threads on 148 KiB of dynamic LDS: the per-kernel limit is raised once per device (host-side
// attribute, no device work).
static int launch_instance(const void* fn, int64_t blocks, void* arg, hipStream_t stream, const char* what) {
    const size_t lds = kLdsFloats * sizeof(float);
    static PerDeviceOnce attr_once;
    const int arc = attr_once.run([&]() {
        for (const auto& row : kKernels)
            for (const void* f : row) {
                if (!f) continue;
                const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
                if (e != hipSuccess) { set_error("hipFuncSetAttribute: %s", hipGetErrorString(e)); return -2; }
            }
        return 0;
    });
    if (arc) return arc;
    void* args[] = {arg};
    (void)hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(256), args, lds, stream);
    return check_launch(what);
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
    if (is_depth_kind(kind) && (a.film_depth != film_depth(kind) || !a.film)) {
        set_error("FiLM depth kind 0x%x launched without its depth or table", kind);
        return -1;
    }
    const int row = is_depth_kind(kind) ? kFilmDepthRow + film_use_dir(kind) : kind;
    return launch_instance(kKernels[row][sigma_only ? FWD_SIGMA : a.save ? FWD_SAVE : FWD_INFER], blocks, const_cast<MlpArgs*>(&a), stream,
                           "field_mlp_fwd");
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
    return launch_instance(kKernels[kind][FWD_SIGMA_WINDOW], blocks, const_cast<MlpArgs*>(&a), stream, "field_mlp_fwd_window");
}

int launch_mlp_list(int kind_in, const MlpArgs& a_in, const int* list, const int* count, hipStream_t stream) {
    const int kind = canon_kind(kind_in);
    if (bad_kind(kind)) return -1;
    if (!has_list_kernel(kind) || (a_in.save && a_in.save_points < a_in.points_per_group) || a_in.film || a_in.mode != 1 || a_in.n_samples < 1 || !list || !count ||
        a_in.points_per_group < 1 || a_in.points_per_group > 0x7fffffffLL ||
        a_in.points_per_group != a_in.rays_per_group * a_in.n_samples) {
        set_error("kind %d: bad list-driven launch", kind);
        return -1;
    }
    MlpArgs a = a_in;
    a.live_rays = list; a.live_count = count;
    const int64_t blocks = (a.points_per_group + 127) / 128;           // worst case: every point listed
    return launch_instance(kKernels[kind][a.save ? FWD_LIST_SAVE : FWD_LIST], blocks, &a, stream, "field_mlp_fwd_list");
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
    return 0;
}

int launch_mlp_trunk_spill(int kind, const MlpArgs& a, const DeferArgs& d, hipStream_t stream) {
    if (const int rc = check_deferred(kind, a, d)) return rc;
    DeferMlpArgs da{a, d};
    return launch_instance(kKernels[kind][FWD_SPILL], a.tiles_per_group, &da, stream, "field_mlp_trunk_spill");
}

int launch_mlp_colour(int kind, const MlpArgs& a, const DeferArgs& d, hipStream_t stream) {
    if (const int rc = check_deferred(kind, a, d)) return rc;
    // one block per CU (148 KiB of LDS each) strides over the tiles below the device count; never more blocks than tiles
    const int cus = compute_units();
    if (cus < 1) return -2;
    const int64_t blocks = a.tiles_per_group < cus ? a.tiles_per_group : cus;
    DeferMlpArgs da{a, d};
    return launch_instance(kKernels[kind][FWD_COLOUR], blocks, &da, stream, "field_mlp_colour");
}

}  // namespace mi
