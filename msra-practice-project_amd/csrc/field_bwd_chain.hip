// field_bwd_chain.hip - the backward CHAIN kernels of the fused field MLP (gfx950), one per field kind, and their launcher
// (field_bwd.h: the overview of the backward and what this unit shares with field_bwd_dw.hip).
//
// These kernels are the most register-sensitive code of the library; the comments in them record the spills found and
// removed.  Their text, and that of every device helper they call, is FROZEN: a change to it comes with its own measurement
// (DESIGN.md 4.3), which is why the weight-gradient engines, the planner and the orchestration live in another unit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "field_bwd.h"
#include "field_kinds.h"
#include "field_mlp_device.h"

#include <type_traits>

namespace mi {

#ifdef MI_PROFILE_STAMPS
unsigned long long* g_bwd_stamps = nullptr;       // set by mi_debug_set_stamps (api.hip), diagnostic build only
#endif

// f32x4 element i of a lane's row in a [point][width] region: a UNIFORM base pointer (SGPR pair) + one per-lane 32-bit
// byte offset (+ 16 i as the instruction's immediate) - the `global_load/store v, v_off, s[base:base+1] offset:imm` form.
template <class V>
struct RowRef {
    using Byte = std::conditional_t<std::is_const_v<V>, const char, char>;
    Byte* base;
    uint32_t off;
    __device__ __forceinline__ V& operator[](int i) const {
        return *reinterpret_cast<V*>(base + (uint64_t)off + (uint64_t)((uint32_t)i * 16u));
    }
};

// The saved row of the chain's first epilogue (the 128-wide dir layer), loaded at the top of the kernel: its latency
// overlaps the first weight stage's DMA and the head gradients instead of following them.
template <int MB>
__device__ __forceinline__ void load_saved_row(f32x4 (&sv)[MB * 4], const float* __restrict__ rows, int64_t ld, int64_t p, int h) {
    const f32x4* row = reinterpret_cast<const f32x4*>(rows + p * ld + 4 * h);
#pragma unroll
    for (int j = 0; j < MB * 4; ++j) sv[j] = row[(j / 4) * 8 + (j % 4) * 2];
}

// A lane's switch words of a ReLU layer (field_layout.h nerf_acts() 12..: MB / 2 dwords per (point, half)), one load
template <int MB>
__device__ __forceinline__ void load_switches(uint32_t (&mw)[4], const float* __restrict__ sw, int64_t p, int h) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(sw) + (p * 2 + h) * (MB / 2);
    if constexpr (MB == 8) { const uint4 v = *reinterpret_cast<const uint4*>(src); mw[0] = v.x; mw[1] = v.y; mw[2] = v.z; mw[3] = v.w; }
    else { const uint2 v = *reinterpret_cast<const uint2*>(src); mw[0] = v.x; mw[1] = v.y; mw[2] = 0u; mw[3] = 0u; }
}

// dA = dX (.) relu'(H): the layer's switch bits (`mw`, load_switches) ANDed onto dX; stores dA rows and leaves them in X.
template <int MB>
__device__ __forceinline__ void relu_bwd_store(const f32x16 (&dX)[8], f32x16 (&X)[8], const uint32_t (&mw)[4],
                                               float* __restrict__ dA, int64_t ld, int64_t p, int h) {
    f32x4* drow = reinterpret_cast<f32x4*>(dA + p * ld + 4 * h);
    static_for<MB>([&](auto mc) {
        constexpr int m = decltype(mc)::value;
        static_for<4>([&](auto rc) {
            constexpr int rg = decltype(rc)::value;
            f32x4 o;
            o.x = __uint_as_float(__float_as_uint(dX[m][4 * rg + 0]) & relu_switch_of<m, rg, 0>(mw));
            o.y = __uint_as_float(__float_as_uint(dX[m][4 * rg + 1]) & relu_switch_of<m, rg, 1>(mw));
            o.z = __uint_as_float(__float_as_uint(dX[m][4 * rg + 2]) & relu_switch_of<m, rg, 2>(mw));
            o.w = __uint_as_float(__float_as_uint(dX[m][4 * rg + 3]) & relu_switch_of<m, rg, 3>(mw));
            X[m][4 * rg + 0] = o.x; X[m][4 * rg + 1] = o.y; X[m][4 * rg + 2] = o.z; X[m][4 * rg + 3] = o.w;
            drow[m * 8 + rg * 2] = o;
        });
    });
}

// Head gradients of point p (rgb = sigmoid(pre), sigma = relu(pre)): dL/d(pre) from the forward outputs and their gradients.
// The caller stores them to its kind's heads region ([points][4]: rgb 0..2, sigma 3).
struct HeadGrads { float d0, d1, d2, ds; };
// (p: the row of raw / g_raw - the point's own, or list[e] of a counted launch)
__device__ __forceinline__ HeadGrads head_grads(const BwdArgs& a, int64_t p) {
    const f32x4 g = reinterpret_cast<const f32x4*>(a.g_raw)[p];
    const f32x4 o = reinterpret_cast<const f32x4*>(a.raw)[p];
    const float d0 = g.x * o.x * (1.f - o.x), d1 = g.y * o.y * (1.f - o.y), d2 = g.z * o.z * (1.f - o.z);
    const float ds = o.w > 0.f ? g.w : 0.f;
    return {d0, d1, d2, ds};
}

// One backward-chain layer with everything but the MFMAs sliced between them (mma_chunk's hooks):
//   pre(m, part)  : accumulator start, s * aux row `piece` of slot `aux_slot` (SCALED: the sigma head's contribution), else
//                   nothing: the layer's first MFMAs take srcC = 0;
//   mid(kb, slot) : the layer's row traffic, spread over its K blocks (below);
//   post(m, part) : dA = dX (.) act'(saved), left in X as the next layer's B operand.
// B operands come from bsel; when the last K block reads X[j] with j < MB-1 pass a copy (post overwrites X[j]).
// The three epilogues:
//   EPI_LINEAR : dA = dX; `saved` is not read.
//   EPI_RELU   : `saved` is the layer's SWITCH region (one bit per unit, MB / 2 dwords per lane: one load in the layer's
//                first mid slot); dA = dX with the switched-off units cleared.
//   EPI_SIN    : `saved` = the layer's X rows with the cosine's sign in the lowest mantissa bit; the derivative factor
//                C = 30 cos(30 u) is rebuilt from them (mi_math.h:dsin30_from_saved_x4) one K block after the quarter's load
//                was issued, in the mid slot that issues a later quarter's load; dA = dX (.) C.
// Row stores are NOT guarded: lanes past the end of a partial tile are clamped to its last point, compute what that
// point's own lane computes and store the same bytes to the same address; a guard costs a saveexec / branch / restore
// around every store and stalled the in-order wave for hundreds of cycles each (field_mlp_device.h:fwd_layer).
// Row traffic is spread over the layer instead of bursting in one row (32 x 1 KiB per wave inside 2048 cycles
// saturates the CU's vector-memory path and stalls the in-order wave): the saved-row quarters are loaded one per mid
// slot, K blocks ahead of the epilogue that needs them - 8-K-block layers: quarter j in slot 4(j%6) of K block 1 + j/6;
// 4-K-block layers: slot 2(j%8) of K block j/8 - and with DEFER the dA rows this layer produces are not stored by its own
// epilogue but by the NEXT layer's mid slots (slot 4(j%4)+2 of K block j/4, resp. 2(j%8)+1 of K block j/8; they sit
// unchanged in X, that layer's B operand, until its last row) - PREV_MB blocks to `prev_dA`.
// The FiLM chain has a layer of its own (film_chain_layer): it stores dL/du but carries gamma (.) dL/du.
enum BwdEpi : int { EPI_LINEAR = 0, EPI_RELU = 1, EPI_SIN = 2 };
constexpr int kNoStart = 0;      // `piece` of a layer that is not SCALED: never read

template <int KB, int MB, int NEXT_AUX, int NEXT_BLOCK, int EPI, bool SCALED, bool DEFER = false, int PREV_MB = 0, class BSel>
__device__ __forceinline__ void bwd_layer(Ctx& c, int aux_slot, int piece, float s, BSel bsel, f32x16 (&acc)[8],
                                          f32x16 (&X)[8], float* __restrict__ dA, int64_t ld, int64_t p,
                                          const float* __restrict__ saved = nullptr, float* __restrict__ prev_dA = nullptr,
                                          int64_t prev_ld = 0) {
    static_assert(KB >= 4, "four K blocks are the fewest whose mid slots carry the 32 row quarters");
    static_assert(KB != 8 || MB == 8, "the 8-K-block slot mapping below counts on 24 mid slots per K block (MB = 8)");
    const int h = c.h;
    // only SCALED layers read the start row: lds_base's opaque asm would otherwise keep a dead address alive across a
    // layer loop (the SirenNeRF chain spilled and reloaded exactly that, once per layer, in front of a stage barrier)
    lds4_t pv = nullptr;
    if constexpr (SCALED) pv = lds_base(c.smem + kLdsAux0 + aux_slot * kLdsAux + h * 16);
    // Row addresses as a UNIFORM base (the tile's first point: SGPRs) plus one 32-bit byte offset per lane (the lane's
    // point inside the tile: < 128 rows), so a row instruction is `global_load/store ..., v_off, s[base]` and the three
    // row pointers of a layer cost one VGPR, not three 64-bit pairs: round 4 - the SirenNeRF chain kept its per-lane
    // 64-bit row pointers across the layer loop in scratch (6 spilled registers, 3 reloads per layer, each followed by an
    // s_waitcnt vmcnt(0) that drains the wave's row traffic).
    const int64_t tile0 = (int64_t)blockIdx.x * 128;
    const uint32_t lrow = (uint32_t)(p - tile0);
    const RowRef<const f32x4> srow{reinterpret_cast<const char*>(saved + tile0 * ld), (lrow * (uint32_t)ld + 4u * h) * 4u};
    const RowRef<f32x4> drow{reinterpret_cast<char*>(dA + tile0 * ld), (lrow * (uint32_t)ld + 4u * h) * 4u};
    const RowRef<f32x4> prow{reinterpret_cast<char*>(prev_dA + tile0 * prev_ld), (lrow * (uint32_t)prev_ld + 4u * h) * 4u};
    // ReLU layers: `saved` is the layer's SWITCH region (one bit per unit, MB / 2 dwords per lane: one load in the layer's
    // first mid slot) - round 4; sin layers: the saved X rows, a quarter per slot, decoded one K block later
    f32x4 sv[(EPI == EPI_LINEAR || EPI == EPI_RELU) ? 1 : MB * 4];
    uint32_t mw[4] = {0u, 0u, 0u, 0u};
    const auto pre = [&](auto mc, auto pc) {
        constexpr int m = decltype(mc)::value, rg = decltype(pc)::value;
        if constexpr (SCALED) {
            const f32x4 w = pv[piece * 64 + m * 8 + rg];
            acc[m][4 * rg + 0] = w.x * s; acc[m][4 * rg + 1] = w.y * s; acc[m][4 * rg + 2] = w.z * s; acc[m][4 * rg + 3] = w.w * s;
        }       // else: nothing to write, the layer's first MFMAs take srcC = 0 (mma_layer_fn ZERO_START)
    };
    static_assert(EPI != EPI_SIN || KB >= 5, "sin rows are decoded one K block after their load");
    const auto mid = [&](auto kbc, auto sc) {
        constexpr int kb = decltype(kbc)::value, slot = decltype(sc)::value, j = kb * 8 + slot / 2;
        if constexpr (KB == 8) {
            // 8 K blocks: the row traffic is spread over the whole layer (tools/probes/mfma_store_mix.hip: 8 + 8 quarters
            // per K block run into a mixed read/write ceiling - 80-110 cycles per instruction instead of 17-33 - and
            // half that density costs a quarter as much).  Loads: slots 0, 4, .., 20 of K blocks 1..6, decoded one K block
            // later (K block 7: slots 0 and 4); deferred stores: slots 2, 6, 10, 14 of K blocks 0..7.
            if constexpr ((slot & 3) == 0) {
                // K blocks 1..6 (not 0..5): the saved rows are needed by the layer's LAST row only, and every K block
                // they arrive later is a K block in which 24 registers stay free while all of X is still live (round 3:
                // siren_bwd_kernel spilled 6 registers, and each scratch reload drains the wave's row traffic)
                constexpr int jl = (kb - 1) * 6 + slot / 4;
                if constexpr (EPI == EPI_SIN && kb >= 2 && jl - 6 >= 0 && jl - 6 < MB * 4) {
                    sv[jl - 6] = dsin30_from_saved_x4(sv[jl - 6]);
                }
                if constexpr (EPI == EPI_SIN && kb >= 1 && kb < 7 && jl < MB * 4) sv[jl] = srow[(jl / 4) * 8 + (jl % 4) * 2];
                if constexpr (EPI == EPI_RELU && kb == 1 && slot == 0) load_switches<MB>(mw, saved, p, h);
            } else if constexpr ((slot & 3) == 2 && slot < 16) {
                constexpr int js = kb * 4 + slot / 4;
                if constexpr (js < PREV_MB * 4) {
                    constexpr int m = js / 4, rg = js % 4;
                    prow[m * 8 + rg * 2] = f32x4{X[m][4 * rg + 0], X[m][4 * rg + 1], X[m][4 * rg + 2], X[m][4 * rg + 3]};
                }
            }
        } else
        if constexpr (EPI == EPI_SIN && kb >= 1 && kb < 5 && slot < 16 && (slot & 1) == 0 && j - 8 < MB * 4) {
            sv[j - 8] = dsin30_from_saved_x4(sv[j - 8]);
        }
        if constexpr (KB != 8 && kb < 4 && slot < 16) {          // 4 K blocks: all 16 mid slots of rows 1-2 are needed
            if constexpr ((slot & 1) == 0) {
                if constexpr (EPI == EPI_SIN && j < MB * 4) sv[j] = srow[(j / 4) * 8 + (j % 4) * 2];
                if constexpr (EPI == EPI_RELU && j == 0) load_switches<MB>(mw, saved, p, h);
            } else if constexpr (j < PREV_MB * 4) {
                constexpr int m = j / 4, rg = j % 4;
                prow[m * 8 + rg * 2] = f32x4{X[m][4 * rg + 0], X[m][4 * rg + 1], X[m][4 * rg + 2], X[m][4 * rg + 3]};
            }
        }
    };
    const auto post = [&](auto mc, auto pc) {
        constexpr int m = decltype(mc)::value, rg = decltype(pc)::value;
        f32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float d = acc[m][4 * rg + q];
            if constexpr (EPI == EPI_RELU) {
                const uint32_t on = q == 0 ? relu_switch_of<m, rg, 0>(mw) : q == 1 ? relu_switch_of<m, rg, 1>(mw)
                                  : q == 2 ? relu_switch_of<m, rg, 2>(mw) : relu_switch_of<m, rg, 3>(mw);
                o[q] = __uint_as_float(__float_as_uint(d) & on);
            } else if constexpr (EPI == EPI_SIN) o[q] = sv[m * 4 + rg][q] * d;
            else o[q] = d;
            X[m][4 * rg + q] = o[q];
        }
        if constexpr (!DEFER) drow[m * 8 + rg * 2] = o;
    };
    // a layer that stores its own dA rows (the chain's last one: there is no next layer to do it) runs its last K block
    // m-major, so the 32 row stores of the epilogue are spread over 128 MFMAs instead of bursting out of the last 32
    // (stamped profile, round 3: the FiLM chain's last layer took 89.5 k cycles where the others take 76-78 k)
    mma_layer_fn<KB, MB, NEXT_AUX, NEXT_BLOCK, false, !SCALED, !DEFER>(c, aux_slot, 0, bsel, acc, pre, post, mid);
}

// =========================================================================================
// NeRF / TinyNeRF backward chain (reverse of nerf/nerf.py:75-94)
// =========================================================================================
template <bool TINY, bool COUNTED = false>
__global__ __launch_bounds__(256, 1) void nerf_bwd_kernel(std::conditional_t<COUNTED, CountedBwdArgs, BwdArgs> a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int64_t rows = a.points;                     // rows of the launch; P below stays the regions' stride
    if constexpr (COUNTED) {
        rows = counted_rows(a.count, a.points);
        if ((int64_t)blockIdx.x * 128 >= rows) return;      // before any LDS DMA
    }
    Ctx c = make_ctx_raw(smem, a.packed, nullptr);
    constexpr RegionLayout AL = TINY ? tiny_acts() : nerf_acts();
    constexpr RegionLayout GL = TINY ? tiny_grads() : nerf_grads();
    // Backward segment 0 is the dir layer's (the rgb head's rows in front of it; TinyNeRF: and the sigma head's), segment i
    // the layer's i layers further back: S the one whose start takes the sigma head's row, N - 1 the chain's last (layers_pos.1).
    constexpr FieldKind K = kFieldKinds[TINY ? MI_FIELD_TINY_NERF : MI_FIELD_NERF];
    constexpr Segments B = segments(K.bwd);
    constexpr int N = B.n, S = TINY ? 0 : 1;
    constexpr int kRgbRow = B.seg[0].piece(AUX_WROW, K.rgb_head()), kSigmaRow = B.seg[S].piece(AUX_WROW, K.sigma_head);
    static_assert(kRgbRow >= 0 && kSigmaRow >= 0, "the heads' rows ride in front of the layers whose input gradient they start");
    static_assert(B.seg[0].piece(AUX_WROW, K.rgb_head(), 1) == kRgbRow + 1 && B.seg[0].piece(AUX_WROW, K.rgb_head(), 2) == kRgbRow + 2,
                  "the rgb head's three rows are consecutive pieces: the W_rgb^T loop below reads kRgbRow + 0..2");
    constexpr int kDirBlocks = 4, kXBlocks = 8;             // K blocks the B-operand selectors below serve
    static_assert(N == (TINY ? 4 : 9) && B.blocks(0) == kDirBlocks && B.blocks(1) == kXBlocks && B.uniform(TINY ? 1 : 2, N - 2) &&
                      B.blocks(N - 2) == kXBlocks && B.blocks(N - 1) == kXBlocks,
                  "the layers this kernel spells out are the whole chain; the plain ones have one shape, and K blocks for all of X");
    const int64_t P = a.points;
    issue_first_stage<B.aux(0), B.block_pieces(0), false>(c, 0);

    const int64_t local = (int64_t)blockIdx.x * 128 + c.wave * 32 + (c.lane & 31);
    const bool valid = local < rows;
    const int64_t p = valid ? local : rows - 1;
    int64_t q = p;                               // row of raw / g_raw
    if constexpr (COUNTED) q = a.list[p];
    const HeadGrads hg = head_grads(a, q);
    const float ds = hg.ds;
    if (valid && c.h == 0) reinterpret_cast<f32x4*>(a.grads + (int64_t)region_offset(GL, GL.n - 1) * P)[p] = f32x4{hg.d0, hg.d1, hg.d2, ds};

    f32x16 X[kXBlocks], acc[8];
    const auto sel_x = [&](auto kb) -> const f32x16& { return X[decltype(kb)::value]; };
    const auto acts = [&](int region) { return a.acts + (int64_t)region_offset(AL, region) * P; };
    const auto grads = [&](int region) { return a.grads + (int64_t)region_offset(GL, region) * P; };
    // ReLU switches (one bit per unit) of layer H_l: region SW0 + l - 1, of the dir layer H_d: the last region
    constexpr int SW0 = AL.relu_switch0();
    const auto sw = [&](int l) { return a.acts + ((int64_t)region_offset(AL, SW0) + 8 * (l - 1)) * P; };
    uint32_t hsw[4];
    load_switches<4>(hsw, acts(AL.n - 1), p, c.h);
    MI_STAMP(a, 0);

    __syncthreads();                                        // head rows (and K block 0) have landed
    {   // dH_d = W_rgb^T d_pre_rgb (128 features); the head's three rows are consecutive aux pieces of slot 0
        const lds4_t pw = lds_base(smem + kLdsAux0 + c.h * 16);
#pragma unroll
        for (int m = 0; m < kDirBlocks; ++m)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                const f32x4 w0 = pw[(kRgbRow + 0) * 64 + m * 8 + rg], w1 = pw[(kRgbRow + 1) * 64 + m * 8 + rg], w2 = pw[(kRgbRow + 2) * 64 + m * 8 + rg];
                acc[m][4 * rg + 0] = fmaf(w2.x, hg.d2, fmaf(w1.x, hg.d1, w0.x * hg.d0));
                acc[m][4 * rg + 1] = fmaf(w2.y, hg.d2, fmaf(w1.y, hg.d1, w0.y * hg.d0));
                acc[m][4 * rg + 2] = fmaf(w2.z, hg.d2, fmaf(w1.z, hg.d1, w0.z * hg.d0));
                acc[m][4 * rg + 3] = fmaf(w2.w, hg.d2, fmaf(w1.w, hg.d1, w0.w * hg.d0));
            }
    }
    relu_bwd_store<kDirBlocks>(acc, X, hsw, grads(TINY ? 4 : 9), 128, p, c.h);            // dA of the dir layer
    MI_STAMP(a, 1);

    int slot = 0;
    if constexpr (!TINY) {
        // layers_dir[1]^T: dG = W[:, :256]^T dA (K = 128); layers_dir[0] is linear: dA = dG.  The B operand is a
        // copy: the epilogue rewrites X[0..3] while the last K block still reads X[3].
        f32x16 Bd[kDirBlocks];
#pragma unroll
        for (int m = 0; m < kDirBlocks; ++m) Bd[m] = X[m];
        const auto sel_d = [&](auto kb) -> const f32x16& { return Bd[decltype(kb)::value]; };
        bwd_layer<B.blocks(0), B.mb(0), B.aux(1), B.block_pieces(1), EPI_LINEAR, false, true, 0>(c, slot, kNoStart, 0.f, sel_d, acc, X, grads(8), 256, p);
        MI_STAMP(a, 2);
        slot ^= 1;
        // layers_dir[0]^T, plus the sigma head's contribution to dH8; dA7 = dH8 (.) [H8>0]
        bwd_layer<B.blocks(1), B.mb(1), B.aux(2), B.block_pieces(2), EPI_RELU, true, true, B.mb(0)>(c, slot, kSigmaRow, ds, sel_x, acc, X, grads(7), 256, p,
                                                                                                    sw(8), grads(8), 256);
        MI_STAMP(a, 3);
        slot ^= 1;
#ifdef MI_PROFILE_STAMPS
        if (a.stamps) c.rowst = a.stamps + (int64_t)blockIdx.x * 128 + 32;                     // rows of L7^T: 32..64
#endif
        bwd_layer<B.blocks(2), B.mb(2), B.aux(3), B.block_pieces(3), EPI_RELU, false, true, B.mb(1)>(c, slot, kNoStart, 0.f, sel_x, acc, X, grads(6), 256, p,
                                                                                                     sw(7), grads(7), 256);  // L7^T
#ifdef MI_PROFILE_STAMPS
        if (c.rowst) { MI_ROW_STAMP(c); }
        c.rowst = nullptr;
#endif
        MI_STAMP(a, 4);
        bwd_layer<B.blocks(2), B.mb(2), B.aux(3), B.block_pieces(3), EPI_RELU, false, true, B.mb(1)>(c, slot, kNoStart, 0.f, sel_x, acc, X, grads(5), 256, p,
                                                                                                     sw(6), grads(6), 256);  // L6^T
        MI_STAMP(a, 5);
        bwd_layer<B.blocks(2), B.mb(2), B.aux(3), B.block_pieces(3), EPI_RELU, false, true, B.mb(1)>(c, slot, kNoStart, 0.f, sel_x, acc, X, grads(4), 256, p,
                                                                                                     sw(5), grads(5), 256);  // L5^T (h part)
        MI_STAMP(a, 6);
#pragma unroll 1
        for (int l = 4; l >= 2; --l)                                                           // L4^T .. L2^T
            bwd_layer<B.blocks(2), B.mb(2), B.aux(3), B.block_pieces(3), EPI_RELU, false, true, B.mb(1)>(
                c, slot, kNoStart, 0.f, sel_x, acc, X, a.grads + (int64_t)(256 * (l - 1)) * P, 256, p, sw(l), a.grads + (int64_t)(256 * l) * P, 256);
        MI_STAMP(a, 7);                                                                        // after L4^T .. L2^T
        bwd_layer<B.blocks(N - 1), B.mb(N - 1), B.aux(N), B.block_pieces(N), EPI_RELU, false, false, B.mb(N - 2)>(c, slot, kNoStart, 0.f, sel_x, acc, X,
                                                                                                              grads(0), 256, p, sw(1), grads(1), 256);   // L1^T
        MI_STAMP(a, 8);
    } else {
        // dir layer^T with the sigma head's contribution to dH4 (the sigma row rides behind the rgb rows in aux slot 0)
        f32x16 Bd[kDirBlocks];
#pragma unroll
        for (int m = 0; m < kDirBlocks; ++m) Bd[m] = X[m];
        const auto sel_d = [&](auto kb) -> const f32x16& { return Bd[decltype(kb)::value]; };
        bwd_layer<B.blocks(0), B.mb(0), B.aux(1), B.block_pieces(1), EPI_RELU, true, true, 0>(c, 0, kSigmaRow, ds, sel_d, acc, X, grads(3), 256, p, sw(4));
        bwd_layer<B.blocks(1), B.mb(1), B.aux(2), B.block_pieces(2), EPI_RELU, false, true, B.mb(0)>(c, slot, kNoStart, 0.f, sel_x, acc, X, grads(2), 256, p,
                                                                                                     sw(3), grads(3), 256);  // L3^T
        bwd_layer<B.blocks(2), B.mb(2), B.aux(3), B.block_pieces(3), EPI_RELU, false, true, B.mb(1)>(c, slot, kNoStart, 0.f, sel_x, acc, X, grads(1), 256, p,
                                                                                                     sw(2), grads(2), 256);  // L2^T
        bwd_layer<B.blocks(N - 1), B.mb(N - 1), B.aux(N), B.block_pieces(N), EPI_RELU, false, false, B.mb(N - 2)>(c, slot, kNoStart, 0.f, sel_x, acc, X,
                                                                                                              grads(0), 256, p, sw(1), grads(1), 256);   // L1^T
    }
}

// dA = dX (.) C with C = 30 cos(30 A) rebuilt from the saved (sign-encoded) X rows; stores dA rows, leaves them in X.
template <int MB>
__device__ __forceinline__ void sin_bwd_store(const f32x16 (&dX)[8], f32x16 (&X)[8], const f32x4 (&xsv)[MB * 4],
                                              float* __restrict__ dA, int64_t ld, int64_t p, int h) {
    f32x4* drow = reinterpret_cast<f32x4*>(dA + p * ld + 4 * h);
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
            const f32x4 o = dsin30_from_saved_x4(xsv[m * 4 + rg]) *
                            f32x4{dX[m][4 * rg + 0], dX[m][4 * rg + 1], dX[m][4 * rg + 2], dX[m][4 * rg + 3]};
            X[m][4 * rg + 0] = o.x; X[m][4 * rg + 1] = o.y; X[m][4 * rg + 2] = o.z; X[m][4 * rg + 3] = o.w;
            drow[m * 8 + rg * 2] = o;
        }
}

// =========================================================================================
// SirenNeRF backward chain (reverse of nerf/nerf.py:153-170); same shape as NeRF's, sin derivatives
// =========================================================================================
template <bool COUNTED = false>
__global__ __launch_bounds__(256, 1) void siren_bwd_kernel(std::conditional_t<COUNTED, CountedBwdArgs, BwdArgs> a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int64_t rows = a.points;                     // as in nerf_bwd_kernel
    if constexpr (COUNTED) {
        rows = counted_rows(a.count, a.points);
        if ((int64_t)blockIdx.x * 128 >= rows) return;
    }
    Ctx c = make_ctx_raw(smem, a.packed, nullptr);
    constexpr RegionLayout AL = siren_acts();
    constexpr RegionLayout GL = siren_grads();
    // backward segments as in nerf_bwd_kernel: 0 layers_dir.1's (rgb rows in front), 1 layers_dir.0's (sigma row), N - 1 the last
    constexpr FieldKind K = kFieldKinds[MI_FIELD_SIREN_NERF];
    constexpr Segments B = segments(K.bwd);
    constexpr int N = B.n;
    constexpr int kRgbRow = B.seg[0].piece(AUX_WROW, K.rgb_head()), kSigmaRow = B.seg[1].piece(AUX_WROW, K.sigma_head);
    static_assert(kRgbRow >= 0 && kSigmaRow >= 0, "the heads' rows ride in front of the layers whose input gradient they start");
    static_assert(B.seg[0].piece(AUX_WROW, K.rgb_head(), 1) == kRgbRow + 1 && B.seg[0].piece(AUX_WROW, K.rgb_head(), 2) == kRgbRow + 2,
                  "the rgb head's three rows are consecutive pieces: the W_rgb^T loop below reads kRgbRow + 0..2");
    constexpr int kDirBlocks = 4, kXBlocks = 8;             // K blocks the B-operand selectors below serve
    static_assert(N == 9 && B.blocks(0) == kDirBlocks && B.blocks(1) == kXBlocks && B.uniform(2, N - 2) && B.blocks(2) == kXBlocks &&
                      B.blocks(N - 1) == kXBlocks,
                  "layers_dir.1, .0, the loop's six and layers_pos.1 are the whole chain; the loop's have one shape, and K blocks for all of X");
    const int64_t P = a.points;
    issue_first_stage<B.aux(0), B.block_pieces(0), false>(c, 0);

    const int64_t local = (int64_t)blockIdx.x * 128 + c.wave * 32 + (c.lane & 31);
    const bool valid = local < rows;
    const int64_t p = valid ? local : rows - 1;
    int64_t q = p;                               // row of raw / g_raw
    if constexpr (COUNTED) q = a.list[p];
    const HeadGrads hg = head_grads(a, q);
    const float ds = hg.ds;
    if (valid && c.h == 0) reinterpret_cast<f32x4*>(a.grads + (int64_t)region_offset(GL, GL.n - 1) * P)[p] = f32x4{hg.d0, hg.d1, hg.d2, ds};

    f32x16 X[kXBlocks], acc[8];
    const auto sel_x = [&](auto kb) -> const f32x16& { return X[decltype(kb)::value]; };
    const auto acts = [&](int region) { return a.acts + (int64_t)region_offset(AL, region) * P; };
    const auto grads = [&](int region) { return a.grads + (int64_t)region_offset(GL, region) * P; };
    f32x4 xsv[kDirBlocks * 4];
    load_saved_row<kDirBlocks>(xsv, acts(10), 128, p, c.h);

    __syncthreads();
    {   // dH_d = W_rgb^T d_pre_rgb (128 features); the head's three rows are consecutive aux pieces of slot 0
        const lds4_t pw = lds_base(smem + kLdsAux0 + c.h * 16);
#pragma unroll
        for (int m = 0; m < kDirBlocks; ++m)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                const f32x4 w0 = pw[(kRgbRow + 0) * 64 + m * 8 + rg], w1 = pw[(kRgbRow + 1) * 64 + m * 8 + rg], w2 = pw[(kRgbRow + 2) * 64 + m * 8 + rg];
                acc[m][4 * rg + 0] = fmaf(w2.x, hg.d2, fmaf(w1.x, hg.d1, w0.x * hg.d0));
                acc[m][4 * rg + 1] = fmaf(w2.y, hg.d2, fmaf(w1.y, hg.d1, w0.y * hg.d0));
                acc[m][4 * rg + 2] = fmaf(w2.z, hg.d2, fmaf(w1.z, hg.d1, w0.z * hg.d0));
                acc[m][4 * rg + 3] = fmaf(w2.w, hg.d2, fmaf(w1.w, hg.d1, w0.w * hg.d0));
            }
    }
    sin_bwd_store<kDirBlocks>(acc, X, xsv, grads(9), 128, p, c.h);                       // dA layers_dir.1 (X_d rows)
    int slot = 0;
    {   // layers_dir.1^T (h part); layers_dir.0 is linear: dA = dG.  B operand copied (see nerf_bwd_kernel).
        f32x16 Bd[kDirBlocks];
#pragma unroll
        for (int m = 0; m < kDirBlocks; ++m) Bd[m] = X[m];
        const auto sel_d = [&](auto kb) -> const f32x16& { return Bd[decltype(kb)::value]; };
        bwd_layer<B.blocks(0), B.mb(0), B.aux(1), B.block_pieces(1), EPI_LINEAR, false, true, 0>(c, slot, kNoStart, 0.f, sel_d, acc, X, grads(8), 256, p);
    }
    slot ^= 1;
    // layers_dir.0^T + sigma head; dA7 = dX8 (.) C8, C_l rebuilt from the saved X_l rows (acts region l)
    bwd_layer<B.blocks(1), B.mb(1), B.aux(2), B.block_pieces(2), EPI_SIN, true, true, B.mb(0)>(c, slot, kSigmaRow, ds, sel_x, acc, X, grads(7), 256, p, acts(8),
                                                                                               grads(8), 256);
#pragma unroll 1
    for (int l = 7; l >= 2; --l)                                                                // L7^T .. L2^T: dA_{l-1} = dX_l (.) C_l
        bwd_layer<B.blocks(2), B.mb(2), B.aux(3), B.block_pieces(3), EPI_SIN, false, true, B.mb(1)>(
            c, slot, kNoStart, 0.f, sel_x, acc, X, a.grads + (int64_t)(256 * (l - 1)) * P, 256, p, a.acts + (int64_t)(8 + 256 * (l - 1)) * P,
            a.grads + (int64_t)(256 * l) * P, 256);
    bwd_layer<B.blocks(N - 1), B.mb(N - 1), B.aux(N), B.block_pieces(N), EPI_SIN, false, false, B.mb(N - 2)>(c, slot, kNoStart, 0.f, sel_x, acc, X, grads(0),
                                                                                                             256, p, acts(1), grads(1), 256);   // L1^T: dA0 = dX1 (.) C1
}

// =========================================================================================
// FilmSirenNeRF backward chain (reverse of pi_GAN/modules.py:101-118).  Layer l: A = W x + b,
// u = gamma A + beta, X = sin(30 u).  dL/du = dX (.) C is what the chain writes (grads region l); it carries
// dA = gamma (.) dL/du to the next layer in registers.  d gamma / d beta / dW / db all come out of the per-image
// sums T_g = sum_p dL/du X_{l-1}^T and s_g = sum_p dL/du (launch_field_backward), so the chain needs neither
// the linear output A nor any cross-lane reduction.
// =========================================================================================
// dU = dX (.) C with C = 30 cos(30 u) rebuilt from the saved (sign-encoded) X rows; leaves dU in X.  Nothing is stored here:
// the first chain layer's mid slots write these rows (film_chain_layer), like every other layer's.
// `cv`: the point's saved X_8 row, loaded by the caller at the top of the kernel (its latency then overlaps the first
// weight stage's DMA and the head gradients instead of following them).
template <int MB>
__device__ __forceinline__ void film_bwd_first(const f32x16 (&dX)[8], f32x16 (&X)[8], const f32x4 (&cv)[32], float w0sq) {
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
            const f32x4 c = dsin_w_from_saved_x4(cv[m * 4 + rg], w0sq);
            const f32x4 o = c * f32x4{dX[m][4 * rg + 0], dX[m][4 * rg + 1], dX[m][4 * rg + 2], dX[m][4 * rg + 3]};
            X[m][4 * rg + 0] = o.x; X[m][4 * rg + 1] = o.y; X[m][4 * rg + 2] = o.z; X[m][4 * rg + 3] = o.w;
        }
}

// One FiLM chain layer j: dX_j = W_{j+1}^T (gamma_{j+1} (.) dU_{j+1}), dU_j = dX_j (.) C_j.
//
// On entry X holds dL/du_{j+1} itself (round 2 carried gamma (.) dL/du in X and parked dL/du in the C registers until the
// next layer stored it: at the layer boundary 128 + 128 such registers were live next to the A fragments, more than the
// 256 architectural VGPRs - the allocator shuffled ~330 values per layer through AGPRs (v_accvgpr_write / read pairs) and
// spilled 25 registers to scratch, and every scratch reload is followed by an s_waitcnt vmcnt(0) that drains ALL the
// wave's outstanding row loads and stores: tools/isa_stats.py).  Now, one K block ahead of its use as
// the B operand, each block of X is first STORED (the dU_{j+1} rows, a quarter per mid slot) and then scaled in place by
// gamma_{j+1} (the FiLM row in LDS slot `gamma_row`, read one slot earlier): block kb + 1 in K block kb's slots
// 1|2|3, 5|6|7, 9|10|11, 13|14|15 (read gamma | store | scale), block 0 in the layer's first hooks.  The same 128
// multiplies per layer as before, no second copy of anything; X[kb] is dead after K block kb, so X shrinks by a block
// per K block while the C quarters arrive (slots 0, 4, .., 20 of K blocks 1..6, decoded one K block later).
// The epilogue leaves dU_j = C_j (.) dX_j in X (LAST: and stores it, there being no next layer to do it).
// FILM_NEXT: the last stage also DMAs FiLM row `next_film_layer` (= j, what layer j - 1 multiplies by) into the film
// slot `issue_slot ^ 1`, the one not being read.
template <int NEXT_BLOCK, bool SCALED, bool FILM_NEXT, bool LAST>
__device__ __forceinline__ void film_chain_layer(Ctx& c, int piece, float s, f32x16 (&acc)[8], f32x16 (&X)[8],
                                                 f32x4 (&ring)[32], const float* __restrict__ C_rows,
                                                 float* __restrict__ dU, float* __restrict__ prev_dU, int64_t p,
                                                 int issue_slot, int next_film_layer, const float* gamma_row) {
    const int h = c.h;
    const lds4_t pv = lds_base(c.smem + kLdsAux0 + h * 16);          // aux slot 0 (the sigma head's row for SCALED)
    const lds4_t pg = lds_base(gamma_row + h * 4);
    const f32x4* srow = reinterpret_cast<const f32x4*>(C_rows + p * 256 + 4 * h);
    f32x4* drow = reinterpret_cast<f32x4*>(dU + p * 256 + 4 * h);
    f32x4* prow = reinterpret_cast<f32x4*>(prev_dU + p * 256 + 4 * h);
    f32x4 gq;                                                        // gamma quarter read one slot ahead of its use
    const auto pre = [&](auto mc, auto pc) {
        constexpr int m = decltype(mc)::value, rg = decltype(pc)::value;
        if constexpr (SCALED) {
            const f32x4 w = pv[piece * 64 + m * 8 + rg];
            acc[m][4 * rg + 0] = w.x * s; acc[m][4 * rg + 1] = w.y * s; acc[m][4 * rg + 2] = w.z * s; acc[m][4 * rg + 3] = w.w * s;
        }       // else: nothing to write, the layer's first MFMAs take srcC = 0 (mma_layer_fn ZERO_START)
        if constexpr (m == 0) {                                      // before the layer's first MFMA: block 0 of X
            const f32x4 g = pg[rg * 2];
            prow[rg * 2] = f32x4{X[0][4 * rg + 0], X[0][4 * rg + 1], X[0][4 * rg + 2], X[0][4 * rg + 3]};
            const f32x4 t = f32x4{X[0][4 * rg + 0], X[0][4 * rg + 1], X[0][4 * rg + 2], X[0][4 * rg + 3]} * g;
            X[0][4 * rg + 0] = t.x; X[0][4 * rg + 1] = t.y; X[0][4 * rg + 2] = t.z; X[0][4 * rg + 3] = t.w;
        }
    };
    const auto mid = [&](auto kbc, auto sc) {
        constexpr int kb = decltype(kbc)::value, slot = decltype(sc)::value;
        if constexpr ((slot & 3) == 0) {
            // C quarters: quarter j = 6 (kb - 1) + slot / 4 in slots 0, 4, .., 20 of K blocks 1..6, decoded one K block later
            // (K block 7 offers slots 0..15: the last two quarters, loaded in K block 6, are decoded in its slots 0 and 4)
            constexpr int j = (kb - 1) * 6 + slot / 4;
            if constexpr (kb >= 2 && j - 6 >= 0 && j - 6 < 32) {
                ring[j - 6] = dsin_w_from_saved_x4(ring[j - 6], c.w0sq);
            }
            if constexpr (kb >= 1 && kb < 7 && j < 32) ring[j] = srow[(j / 4) * 8 + (j % 4) * 2];
        } else if constexpr (kb < 7 && slot < 16) {
            // block kb + 1 of X, quarter rg = slot / 4: gamma read | dU row store | scale in place
            constexpr int m = kb + 1, rg = slot / 4;
            if constexpr ((slot & 3) == 1) gq = pg[m * 8 + rg * 2];
            if constexpr ((slot & 3) == 2)
                prow[m * 8 + rg * 2] = f32x4{X[m][4 * rg + 0], X[m][4 * rg + 1], X[m][4 * rg + 2], X[m][4 * rg + 3]};
            if constexpr ((slot & 3) == 3) {
                const f32x4 t = f32x4{X[m][4 * rg + 0], X[m][4 * rg + 1], X[m][4 * rg + 2], X[m][4 * rg + 3]} * gq;
                X[m][4 * rg + 0] = t.x; X[m][4 * rg + 1] = t.y; X[m][4 * rg + 2] = t.z; X[m][4 * rg + 3] = t.w;
            }
        }
    };
    const auto post = [&](auto mc, auto pc) {
        constexpr int m = decltype(mc)::value, rg = decltype(pc)::value, j = m * 4 + rg;
        const f32x4 o = ring[j] * f32x4{acc[m][4 * rg + 0], acc[m][4 * rg + 1], acc[m][4 * rg + 2], acc[m][4 * rg + 3]};
        X[m][4 * rg + 0] = o.x; X[m][4 * rg + 1] = o.y; X[m][4 * rg + 2] = o.z; X[m][4 * rg + 3] = o.w;
        if constexpr (LAST) drow[m * 8 + rg * 2] = o;
    };
    const auto sel_x = [&](auto kb) -> const f32x16& { return X[decltype(kb)::value]; };
    mma_layer_fn<8, 8, 0, NEXT_BLOCK, FILM_NEXT, !SCALED, LAST>(c, issue_slot, next_film_layer, sel_x, acc, pre, post, mid);
}

// RT_DEPTH: hidden_layers = L at run time (BwdArgs::film_depth, wave-uniform) for the MI_FIELD_FILM_DEPTH kinds; kinds 2 / 3
// keep the literal 8.  FiLM layers 0..L: the chain runs rgb hidden (L), hidden L-2..0 (L-1..1), input_layer (0).
template <bool USE_DIR, bool RT_DEPTH = false>
__global__ __launch_bounds__(256, 1) void film_bwd_kernel(BwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int64_t group = blockIdx.x / a.tiles_per_group;
    const int64_t tile = blockIdx.x % a.tiles_per_group;
    const int L = RT_DEPTH ? __builtin_amdgcn_readfirstlane(a.film_depth) : 8;
    Ctx c = make_ctx_raw(smem, a.packed, a.film + group * ((L + 1) * kFilmRow));
    // fl(w_0^2) of the module's w_0 (pi_GAN/modules.py:11,73) from the backward stream's trailer: the rebuilt derivative
    // factor is +-sqrt(w_0^2 (1 - X^2)); a uniform (scalar) load
    constexpr FieldKind K = kFieldKinds[USE_DIR ? MI_FIELD_FILM_SIREN_NERF : MI_FIELD_FILM_SIREN_NERF_NODIR];
    static_assert(film_body_floats(8, USE_DIR, true) == packed_body_floats(K.bwd));
    const int kBody = film_body_floats(L, USE_DIR, true);
    c.w0sq = a.packed[kBody + 1];
    // The shapes are depth 8's (kinds 2 / 3): segment 0 is hidden_layer_rgb^T's with both heads' rows in front of it, every
    // other one a plain hidden layer's, the last followed by nothing.  Any other depth's stream has the same (field_kinds.h:
    // film_depth_like_8).  film_chain_layer runs 8 K blocks of 8 row blocks: all of X.
    constexpr Segments B = segments(K.bwd);
    constexpr int N = B.n;
    constexpr int kRgbRow = B.seg[0].piece(AUX_WROW, K.rgb_head()), kSigmaRow = B.seg[0].piece(AUX_WROW, K.sigma_head);
    static_assert(kRgbRow >= 0 && kSigmaRow >= 0, "the heads' rows ride in front of the chain's first layer");
    static_assert(B.seg[0].piece(AUX_WROW, K.rgb_head(), 1) == kRgbRow + 1 && B.seg[0].piece(AUX_WROW, K.rgb_head(), 2) == kRgbRow + 2,
                  "the rgb head's three rows are consecutive pieces: the W_rgb^T loop below reads kRgbRow + 0..2");
    constexpr int kXBlocks = 8;
    static_assert(N == 8 && B.uniform(1, N - 2) && B.aux(1) == 0 && B.blocks(0) == kXBlocks && B.mb(0) == kXBlocks && B.blocks(1) == kXBlocks &&
                      B.mb(1) == kXBlocks && B.seg[N - 1].same_shape(B.seg[1]),
                  "one chain layer per segment, each film_chain_layer's 8 x 8 blocks with no aux pieces issued behind it");
    static_assert(!RT_DEPTH || film_segments_ok(USE_DIR), "every depth's stream has depth 8's shapes at depth 8's distances from its ends");
    const int64_t P = a.points;
    // rgb head rows x3, sigma row; K blocks 0-1 of hidden_layer_rgb^T; FiLM row L -> film slot 0 (row r lives in slot (L - r) & 1)
    issue_first_stage<B.aux(0), B.block_pieces(0), true>(c, 0, L);

    const int64_t local = tile * 128 + c.wave * 32 + (c.lane & 31);
    const bool valid = local < a.points_per_group;
    const int64_t p = group * a.points_per_group + (valid ? local : a.points_per_group - 1);
    const HeadGrads hg = head_grads(a, p);
    const float ds = hg.ds;
    if (valid && c.h == 0) reinterpret_cast<f32x4*>(a.grads + (int64_t)((L + 1) * 256) * P)[p] = f32x4{hg.d0, hg.d1, hg.d2, ds};

    f32x16 X[kXBlocks], acc[8];
    const auto film_row = [&](int r) { return smem + kLdsFilm0 + ((L - r) & 1) * kFilmRow; };       // FiLM row r's LDS slot
    const auto C = [&](int l) { return a.acts + (int64_t)(8 + 256 * l) * P; };    // saved X_l rows: C_l is rebuilt from them
    const auto dU = [&](int l) { return a.grads + (int64_t)(256 * l) * P; };
    f32x4 ring[32];                                            // a layer's C quarters, loaded a K block or more ahead
    {   // the first epilogue's rows (X_L) now, while the first weight stage is still on its way
        const f32x4* crow = reinterpret_cast<const f32x4*>(C(L) + p * 256 + 4 * c.h);
#pragma unroll
        for (int j = 0; j < 32; ++j) ring[j] = crow[(j / 4) * 8 + (j % 4) * 2];
    }

    __syncthreads();
    {   // dX_L = W_rgb^T d_pre_rgb (256 features)
        const lds4_t pw = lds_base(smem + kLdsAux0 + c.h * 16);
#pragma unroll
        for (int m = 0; m < kXBlocks; ++m)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                const f32x4 w0 = pw[(kRgbRow + 0) * 64 + m * 8 + rg], w1 = pw[(kRgbRow + 1) * 64 + m * 8 + rg], w2 = pw[(kRgbRow + 2) * 64 + m * 8 + rg];
                acc[m][4 * rg + 0] = fmaf(w2.x, hg.d2, fmaf(w1.x, hg.d1, w0.x * hg.d0));
                acc[m][4 * rg + 1] = fmaf(w2.y, hg.d2, fmaf(w1.y, hg.d1, w0.y * hg.d0));
                acc[m][4 * rg + 2] = fmaf(w2.z, hg.d2, fmaf(w1.z, hg.d1, w0.z * hg.d0));
                acc[m][4 * rg + 3] = fmaf(w2.w, hg.d2, fmaf(w1.w, hg.d1, w0.w * hg.d0));
            }
    }
    MI_STAMP(a, 0);
    film_bwd_first<kXBlocks>(acc, X, ring, c.w0sq);                                                      // hidden_layer_rgb: X = dU_L
    MI_STAMP(a, 1);
    // Chain layer j multiplies by FiLM row j + 1 (slot (L - 1 - j) & 1) and DMAs row j - what layer j - 1 multiplies by -
    // into the other slot.  j = L - 1 starts from the sigma head's row (aux slot 0, behind the rgb head's).
#if defined(MI_PROFILE_STAMPS) && defined(MI_STAMP_LAYER) && MI_STAMP_LAYER == 7
    if (a.stamps) c.rowst = a.stamps + (int64_t)blockIdx.x * 128 + 32;                          // rows of layer 7: 32..64
#endif
    film_chain_layer<B.block_pieces(1), true, true, false>(c, kSigmaRow, ds, acc, X, ring, C(L - 1), dU(L - 1), dU(L), p, 0, L - 1, film_row(L));
#if defined(MI_PROFILE_STAMPS) && defined(MI_STAMP_LAYER) && MI_STAMP_LAYER == 7
    if (c.rowst) { MI_ROW_STAMP(c); }
    c.rowst = nullptr;
#endif
    MI_STAMP(a, 2);
#pragma unroll 1
    for (int j = L - 2; j >= 1; --j) {                                                           // hidden_layers[L-3..0]
#ifdef MI_PROFILE_STAMPS
#if !defined(MI_STAMP_LAYER) || MI_STAMP_LAYER != 7
        if (j == 4 && a.stamps) c.rowst = a.stamps + (int64_t)blockIdx.x * 128 + 32;            // rows of layer j = 4: 32..64
#endif
#endif
        film_chain_layer<B.block_pieces(2), false, true, false>(c, kNoStart, 0.f, acc, X, ring, C(j), dU(j), dU(j + 1), p, (L - 1 - j) & 1, j, film_row(j + 1));
#ifdef MI_PROFILE_STAMPS
        if (c.rowst) { MI_ROW_STAMP(c); }
        c.rowst = nullptr;
        if (threadIdx.x == 0 && a.stamps) a.stamps[(int64_t)blockIdx.x * 128 + 3 + (L - 2 - j)] = __builtin_amdgcn_s_memtime();   // 3..L
#endif
    }
    film_chain_layer<B.block_pieces(N), false, false, true>(c, kNoStart, 0.f, acc, X, ring, C(0), dU(0), dU(1), p, (L - 1) & 1, 0, film_row(1));   // input_layer
    MI_STAMP(a, 9);
}

// ---- host side ---------------------------------------------------------------------------
// One table of instances, [row][variant], like the forward's (field_mlp.hip).  Rows: the fixed kinds, then the run-time-depth
// FiLM instances without / with the direction (MI_FIELD_FILM_DEPTH kinds other than depth 8, which IS kinds 2 / 3).
// Variants: the plain instance and the counted one (the kinds an occupancy grid exists for); null: no such instance.
enum BwdVariant : int { BWD_PLAIN = 0, BWD_COUNTED, BWD_VARIANTS };
constexpr int kFilmDepthRow = MI_FIELD_KINDS;      // + use_dir
static const void* const kBwdKernels[MI_FIELD_KINDS + 2][BWD_VARIANTS] = {
    {(const void*)nerf_bwd_kernel<false>, (const void*)nerf_bwd_kernel<false, true>},     // MI_FIELD_NERF
    {(const void*)siren_bwd_kernel<false>, (const void*)siren_bwd_kernel<true>},          // MI_FIELD_SIREN_NERF
    {(const void*)film_bwd_kernel<true>},                                                 // MI_FIELD_FILM_SIREN_NERF
    {(const void*)film_bwd_kernel<false>},                                                // MI_FIELD_FILM_SIREN_NERF_NODIR
    {(const void*)nerf_bwd_kernel<true>, (const void*)nerf_bwd_kernel<true, true>},       // MI_FIELD_TINY_NERF
    {(const void*)film_bwd_kernel<false, true>},                                          // any depth, no dir
    {(const void*)film_bwd_kernel<true, true>}};                                          // any depth, dir
// the row of a canonical kind (canon_kind: depth 8 has become kind 2 / 3)
static int bwd_row(int kind) { return is_depth_kind(kind) ? kFilmDepthRow + film_use_dir(kind) : kind; }

// Launches one chain kernel over `blocks` tiles.  The dynamic-LDS attribute of every chain instance is set the first time a
// device is seen; the stamps pointer is the diagnostic build's.  `a` is the kernel's whole argument block: a BwdArgs, or the
// CountedBwdArgs it is the base (and so the first bytes) of.
static int launch_chain(const void* kernel, BwdArgs& a, unsigned blocks, const char* what, hipStream_t stream) {
    const size_t lds = kLdsFloats * sizeof(float);
    static PerDeviceOnce attr_once;
    const int arc = attr_once.run([&]() {
        for (const auto& row : kBwdKernels)
            for (const void* f : row)                    // null: a kind without a counted instance
                if (f && hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
                    set_error("hipFuncSetAttribute failed"); return -2;
                }
        return 0;
    });
    if (arc) return arc;
#ifdef MI_PROFILE_STAMPS
    a.stamps = g_bwd_stamps;
#endif
    void* args[] = {&a};
    (void)hipLaunchKernel(kernel, dim3(blocks), dim3(256), args, lds, stream);
    return check_launch(what);
}

int launch_bwd_chain(int kind, BwdArgs& a, unsigned blocks, hipStream_t stream) {
    return launch_chain(kBwdKernels[bwd_row(kind)][BWD_PLAIN], a, blocks, "backward chain", stream);
}
int launch_bwd_chain_counted(int kind, CountedBwdArgs& a, unsigned blocks, hipStream_t stream) {
    const void* const kernel = kBwdKernels[bwd_row(kind)][BWD_COUNTED];
    if (!kernel) { set_error("kind %d has no counted backward", kind); return -1; }
    return launch_chain(kernel, a, blocks, "backward chain (counted)", stream);
}

}  // namespace mi
