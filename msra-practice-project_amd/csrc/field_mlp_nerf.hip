// field_mlp_nerf.hip - the NeRF family of the fused field-MLP forward (design: field_mlp.hip): nerf_fwd_kernel, one
// template for NeRF and TinyNeRF, and the colour-branch kernel of the deferred fine pass.  This unit holds the NeRF family
// and nothing else: its kernels' machine code depends on what shares their translation unit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "field_kinds.h"
#include "field_mlp_device.h"
#include "field_mlp_instances.h"

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

// the rows of the forward's instance table (field_mlp_instances.h)
extern const void* const kNerfRows[2][FWD_VARIANTS] = {
    // MI_FIELD_NERF
    {(const void*)nerf_fwd_kernel<false, false, false>, (const void*)nerf_fwd_kernel<false, true, false>,
     (const void*)nerf_fwd_kernel<false, false, true>, (const void*)nerf_fwd_kernel<false, false, true, true>,
     (const void*)nerf_fwd_kernel<false, false, true, false, true>, (const void*)nerf_colour_kernel<false>,
     (const void*)nerf_fwd_kernel<false, false, false, false, false, true>,
     (const void*)nerf_fwd_kernel<false, true, false, false, false, true>},
    // MI_FIELD_TINY_NERF
    {(const void*)nerf_fwd_kernel<true, false, false>, (const void*)nerf_fwd_kernel<true, true, false>,
     (const void*)nerf_fwd_kernel<true, false, true>, (const void*)nerf_fwd_kernel<true, false, true, true>,
     (const void*)nerf_fwd_kernel<true, false, true, false, true>, (const void*)nerf_colour_kernel<true>,
     (const void*)nerf_fwd_kernel<true, false, false, false, false, true>,
     (const void*)nerf_fwd_kernel<true, true, false, false, false, true>}};

}  // namespace mi
