// field_mlp_bwd.hip - backward of the fused field MLP (gfx950): what autograd does for
// `network(inputs)` inside run_network (reference nerf/render.py:72-74) when train_nerf.py:168 /
// pi_GAN/train.py call loss.backward().
//
// Three kinds of kernels, all fp32:
//   1. backward CHAIN (one per field kind): same structure as the forward - 128 points per workgroup,
//      features on MFMA rows, the accumulators of dX_l = W_l^T dA_l are, after the activation derivative,
//      the B operands of the next (earlier) layer; transposed weights stream through LDS from a second
//      packed stream (field_layout.h build_*_bwd).  It reads the saved layer inputs for the activation
//      derivative and writes dA of every linear layer as [point][feature] rows.
//   2. dW GEMM: dW_l[M,K] = sum_p dA_l[p,:]^T X_l[p,:] - a plain GEMM whose contraction is over POINTS.
//      Features sit on the MFMA lanes (one float4 load per lane gives the operands of four 32-wide blocks
//      straight from the row-major rows, no LDS), each workgroup reduces a slab of points into a full
//      256x256 tile held in accumulators (256 registers per lane), slabs are combined by a second kernel in
//      a fixed order (deterministic, no atomics).  Bias gradients ride along as column sums of dA.
//   3. head gradients (1- and 3-row weights): VALU reduction over point slabs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "field_kinds.h"
#include "field_mlp_device.h"

#include <type_traits>

namespace mi {

struct BwdArgs {
    const float* packed;     // backward stream
    const float* acts;       // saved layer inputs (regions x points)
    float* grads;            // dA regions x points (written here)
    const float* raw;        // [P,4] forward outputs (rgb post-sigmoid, sigma post-ReLU)
    const float* g_raw;      // [P,4] dL/d(raw)
    int64_t points;
    // FiLM kinds: one table [film_depth + 1][512] per group of points_per_group consecutive points
    const float* film;
    float* film_partial;     // unused by the chain (kept so the argument block stays stable)
    int64_t points_per_group, tiles_per_group, n_tiles;
    unsigned long long* stamps;   // diagnostic build (-DMI_PROFILE_STAMPS) only: [block][128] s_memtime values (MI_STAMP)
    int film_depth;          // FiLM kinds: hidden_layers (the run-time-depth chain reads it), else 0
};

// The COUNTED instances (training with an occupancy grid): the rows are the first *count entries of a device-counted list of
// point indices.  acts / grads hold COMPACT rows (row e belongs to point list[e]; a.points = the capacity, the regions'
// stride), raw / g_raw stay [all points of the pass][4] and are read at row list[e].
struct CountedBwdArgs : BwdArgs {
    const int* list;
    const int* count;
};
// rows of a counted launch (block-uniform), never more than the capacity the buffers were sized for
__device__ __forceinline__ int64_t counted_rows(const int* count, int64_t capacity) {
    const int64_t n = __builtin_amdgcn_readfirstlane(__hip_atomic_load(count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    return n < 0 ? 0 : n < capacity ? n : capacity;
}
// The slab length of the counted weight-gradient kernels: the host plans n_slabs from the CAPACITY (BwdBatcher::slabs_for /
// slab_pts_for, as for a plain pass) and sizes the partial records for it; the device cuts the rows it really has into that
// many equal slabs of whole 32-point stages, slab_len = ceil32(ceil(count / n_slabs)).  With count == capacity this is the
// host planner's slab length (n_slabs = ceil(P / slab) gives (n_slabs - 1) slab < P <= n_slabs slab, so ceil(P / n_slabs) <=
// slab, and n_slabs <= the planned slabs gives >=); n_slabs * slab_len >= count always; a slab past the rows is empty and
// writes a zero record.
__host__ __device__ constexpr int counted_slab_pts(int64_t count, int n_slabs) {
    return (int)(((count + n_slabs - 1) / n_slabs + 31) / 32 * 32);
}
struct CountedRows { const int* count; int64_t capacity; int n_slabs; };

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

// FiLM layer finishing for ONE image (group) g.  T[f][k] = sum_{p in g} dL/du[p][f] X[p][k] (tk = 256, or the 3
// raw-input columns), s[f] = sum_{p in g} dL/du[p][f].  Row f per workgroup, column k per thread:
//   dW[f][col0+k]  (+)= gamma[f] T[f][k]                       (+= for g > 0: images are summed in order)
//   d gamma_g[f]   (+)= sum_k W[f][col0+k] T[f][k]  (+ b[f] s[f] with the bias part: A = W x + b)
//   d beta_g[f]      = s[f];   db[f] (+)= gamma[f] s[f]        (bias part only)
constexpr int kMaxFinishJobs = kFilmDepthMax + 2;   // an image's FiLM layers (at most 13) + the dir columns of hidden_layer_rgb
struct FinishJob {
    const float* T; const float* s; const float* W; const float* b; const float* film_row;
    float* dW; float* db; float* dfilm_row;
    int tk, w_ld, col0, bias_part;
};
struct FinishBatch { FinishJob job[kMaxFinishJobs]; int first_group; };

// grid = (256 rows, jobs): every finishing job of one image in ONE launch (round 2: ten launches of 4.6 us per image,
// 320 per C4 step).  A job that adds to a d gamma another job of the same launch WRITES (hidden_layer_rgb's dir columns
// after its h columns: bias_part = 0) runs in the same workgroup right after it - see launch_field_backward.
__global__ __launch_bounds__(256) void film_finish_kernel(FinishBatch fb) {
    __shared__ float red[4];
    const int f = blockIdx.x, k = threadIdx.x;
    const int first_group = fb.first_group;
    // blockIdx.y indexes the jobs with a bias part; a job without one (it ADDS to the d gamma row of the job before it
    // in the table) is chained behind its predecessor here, so the two never race
    int j = 0;
    for (int seen = -1; j < kMaxFinishJobs; ++j)
        if (fb.job[j].T && fb.job[j].bias_part && ++seen == (int)blockIdx.y) break;
    if (j >= kMaxFinishJobs) return;
    for (; j < kMaxFinishJobs && fb.job[j].T; ++j) {
        const FinishJob& q = fb.job[j];
        const float gamma = q.film_row[f];
        float dot = 0.f;
        if (k < q.tk) {
            const float t = q.T[f * q.tk + k];
            float* w = q.dW + (int64_t)f * q.w_ld + q.col0 + k;
            *w = first_group ? gamma * t : *w + gamma * t;
            dot = q.W[(int64_t)f * q.w_ld + q.col0 + k] * t;
        }
        for (int off = 32; off > 0; off >>= 1) dot += __shfl_xor(dot, off);
        __syncthreads();                                   // red[] of the previous job of this chain has been consumed
        if ((k & 63) == 0) red[k >> 6] = dot;
        __syncthreads();
        if (k == 0) {
            float dg = ((red[0] + red[1]) + red[2]) + red[3];
            if (q.bias_part) {
                dg += q.b[f] * q.s[f];
                q.dfilm_row[f] = dg;
                q.dfilm_row[256 + f] = q.s[f];
                q.db[f] = first_group ? gamma * q.s[f] : q.db[f] + gamma * q.s[f];
            } else {
                q.dfilm_row[f] += dg;
            }
        }
        if (j + 1 < kMaxFinishJobs && fb.job[j + 1].T && fb.job[j + 1].bias_part) break;     // the next job is another chain's head
    }
}

// =========================================================================================
// dW GEMM over points: dW[f][k] = sum_p dA[p][f] X[p][k].  Features sit on the MFMA lanes: lane i of wave-tile
// (wm, wk) owns dA features 128*wm + 4*i + c (c = the four 32-wide row blocks) and X features 32*CB*wk + CB*i + d,
// acc[c][d] (+)= A_c (x) B_d per point pair.  Workgroup = 4 waves = tiles (WM x WK) x k-split KS = 4 / (WM*WK).
// partial record (slab) = [TM][TK] row-major tile, then (with_bias) the TM column sums of dA.
// Rows are staged through LDS by DMA (buffer_load ... lds) rather than loaded per lane (the first version: 4 ms
// of a 60 ms step slower):
// a stage = 32 points = one contiguous run of rows of each operand ([point][feature] rows with lda == TM and
// ldx == TK, which holds for every job), double-buffered; the next stage's 1 KiB pieces are issued one per 8
// MFMAs during the first half of the current stage, so they have half a stage (>= 3 us) to land.  Rows past the
// slab's end read as zero (buffer bounds), so ragged slabs need no masking.  Operand fetch is one ds_read_b128
// (conflict-free: 16 consecutive lanes read 16 consecutive float4) per operand and point pair.
constexpr int kGemmStagePts = 32;

// Up to kMaxGemmJobs GEMMs of one tile shape in ONE launch (grid.y = job): every job contracts the same P points, so
// a training step's nine 256x256 weight gradients are one launch of 9 x slabs workgroups instead of nine launches
// of `slabs` - at the 1024-ray batch of nerf/train_nerf.py the step is launch-bound otherwise.
constexpr int kMaxGemmJobs = 12;
struct GemmBatch {
    const float* dA[kMaxGemmJobs];
    const float* X[kMaxGemmJobs];
    float* partial[kMaxGemmJobs];      // one record per slab of TM*TK (+ TM bias sums) floats
    int with_bias[kMaxGemmJobs];
};

// LDS floats one k-split wave parks for the merge (its 4 x CB accumulator blocks + the bias sums), and the dynamic LDS a
// launch needs: the two stage buffers, or the merge area of the (KS - 1) x TILES parked waves if that is larger.
constexpr int gemm_merge_wave_floats(int CB) { return (4 * CB * 16 + 4) * 64; }
// Stage buffers in the ring.  A 256x256 tile runs 256 MFMAs per wave and stage (6.9 us) on 64 KiB of rows: one stage in
// flight while the other is consumed hides the memory latency, and two buffers are all that fit.  The NARROW tiles run 16 -
// 128 MFMAs (0.4 - 3.4 us) on 20 - 48 KiB: with one stage in flight a CU has ~40 KiB outstanding against a loaded HBM latency
// of ~2 us - Little's law caps the chip at ~2.5 TB/s, which is what round 3 measured for them (2.0 - 2.5 TB/s of algorithmic
// bytes at 0.25 - 0.65 MFMA-busy) while they ask for 3.6 - 6 TB/s.  Their stages are small, so the ring holds one or two more.
template <int CB, int WM, int WK>
constexpr int gemm_ring() {
    constexpr size_t stage = (size_t)kGemmStagePts * (128 * WM + 32 * CB * WK) * sizeof(float);
    return stage >= 64 * 1024 ? 2 : (stage > 20 * 1024 ? 3 : 4);
}
template <int CB, int WM, int WK>
constexpr size_t gemm_lds_bytes() {
    constexpr int TILES = WM * WK, KS = 4 / TILES, TM = 128 * WM, TK = 32 * CB * WK;
    constexpr size_t stage = (size_t)gemm_ring<CB, WM, WK>() * kGemmStagePts * (TM + TK) * sizeof(float);
    constexpr size_t merge = (size_t)(KS - 1) * TILES * gemm_merge_wave_floats(CB) * sizeof(float);
    return stage > merge ? stage : merge;
}

// COUNTED: the rows and the slab length come from the device count (counted_slab_pts); a slab past the rows contracts nothing
// (its descriptors bound zero records, its ring reads zeros) and writes a zero record.
template <int CB, int WM, int WK, bool COUNTED = false>
__global__ __launch_bounds__(256, 1) void dw_gemm_kernel(GemmBatch jobs, std::conditional_t<COUNTED, CountedRows, int64_t> rows_in,
                                                         int slab_in) {
    int64_t P;
    int slab_pts;
    if constexpr (COUNTED) {
        P = counted_rows(rows_in.count, rows_in.capacity);
        slab_pts = counted_slab_pts(P, rows_in.n_slabs);
    } else {
        P = rows_in;
        slab_pts = slab_in;
    }
    const float* __restrict__ dA = jobs.dA[blockIdx.y];
    const float* __restrict__ X = jobs.X[blockIdx.y];
    float* __restrict__ partial = jobs.partial[blockIdx.y];
    const int with_bias = jobs.with_bias[blockIdx.y];
    constexpr int TILES = WM * WK, KS = 4 / TILES, TM = 128 * WM, TK = 32 * CB * WK, T = kGemmStagePts;
    constexpr int PA = T * TM / 256, PB = T * TK / 256;              // 1 KiB pieces per stage and operand
    constexpr int NPW = (PA + PB + 3) / 4;                           // pieces per wave and stage
    constexpr int STEPS = (T / 2) / KS;                              // point pairs per wave and stage
    constexpr int PPS = (NPW + STEPS / 2 - 1) / (STEPS / 2);         // pieces issued per step in the first half
    constexpr int STAGE = T * (TM + TK);                             // floats per stage buffer
    typedef float bvec __attribute__((ext_vector_type(CB)));
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = lane & 31, h = lane >> 5;
    const int tile = wave % TILES, ks = wave / TILES;
    const int wm = tile / WK, wk = tile % WK;
    const int64_t p0 = (int64_t)blockIdx.x * slab_pts;
    int64_t p1 = p0 + slab_pts < P ? p0 + slab_pts : P;
    if constexpr (COUNTED) p1 = p1 < p0 ? p0 : p1;                   // an empty slab: zero records, zero stages
    const int n_stages = (int)((p1 - p0 + T - 1) / T);
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)(dA + p0 * TM), 0, (int)((p1 - p0) * TM * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)(X + p0 * TK), 0, (int)((p1 - p0) * TK * 4), 0x00020000);
    // piece q (0..PA+PB-1) of stage st into buffer b; wave w owns pieces w, w+4, ...
    const auto issue = [&](int st, int b, int k) {
        const int q = wave + 4 * k;
        if (q < PA)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (MI_LDS void*)(smem + b * STAGE + q * 256), 16, lane * 16,
                                                     st * (T * TM * 4) + q * 1024, 0, 0);
        else if (q < PA + PB)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, (MI_LDS void*)(smem + b * STAGE + T * TM + (q - PA) * 256), 16,
                                                     lane * 16, st * (T * TK * 4) + (q - PA) * 1024, 0, 0);
    };

    f32x16 acc[4][CB];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int d = 0; d < CB; ++d)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[c][d][r] = 0.f;
    f32x4 bsum = {0.f, 0.f, 0.f, 0.f};

    // Ring of NB stage buffers: stages st+1 .. st+NB-2 are in flight while stage st is consumed, and stage st+NB-1 is
    // issued during it (into the buffer stage st-1 just left).  Every wave issues exactly NPW pieces per stage, ALWAYS -
    // stages past the slab's end read zeros through the buffer bounds and are never consumed - so "stage st has landed" is
    // `s_waitcnt vmcnt((NB - 2) * NPW)`: the wave's vector-memory operations complete in order and nothing else is issued
    // in the loop.
    constexpr int NB = gemm_ring<CB, WM, WK>();
    static_assert((PA + PB) % 4 == 0, "every wave must issue the same number of pieces per stage (the vmcnt arithmetic)");
    static_assert((NB - 2) * NPW < 64, "vmcnt is a 6-bit counter");
#pragma unroll
    for (int sp = 0; sp < NB - 1; ++sp)
#pragma unroll
        for (int k = 0; k < NPW; ++k) issue(sp, sp, k);
    int b = 0;
    for (int st = 0; st < n_stages; ++st) {
        // stage st has landed in every wave's view: own pieces by the count, the others' by the barrier
        asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"((NB - 2) * NPW) : "memory");
        const int bn = b == 0 ? NB - 1 : b - 1;                      // the buffer stage st - 1 used = (st + NB - 1) % NB
        // this wave's first point pair of the stage; step sidx reads rows 2 KS sidx further on (an immediate offset)
        const float* As = smem + b * STAGE + 128 * wm + 4 * i + (2 * ks + h) * TM;
        const float* Bs = smem + b * STAGE + T * TM + 32 * CB * wk + CB * i + (2 * ks + h) * TK;
        // Operands one step ahead: the reads of step s + 1 are issued at the top of step s and pinned there, so their LDS
        // latency runs under the 4 CB MFMAs of step s.  (Left to the scheduler, the A operand of a step was read three MFMAs
        // before the step began with an s_waitcnt lgkmcnt(0) right behind it - the matrix pipe drained at every step: the
        // ISA of round 2's kernel, tools/isa_stats.py.)  Only the first step of a stage waits for LDS.
        f32x4 av = *reinterpret_cast<const f32x4*>(As);
        bvec bv = *reinterpret_cast<const bvec*>(Bs);
        static_for<STEPS>([&](auto sc) {
            constexpr int sidx = decltype(sc)::value;
            f32x4 av_n = av;
            bvec bv_n = bv;
            if constexpr (sidx + 1 < STEPS) {
                av_n = *reinterpret_cast<const f32x4*>(As + 2 * KS * (sidx + 1) * TM);
                bv_n = *reinterpret_cast<const bvec*>(Bs + 2 * KS * (sidx + 1) * TK);
                __builtin_amdgcn_sched_barrier(0);
            }
            bsum += av;
            static_for<4>([&](auto cc) {
                constexpr int c = decltype(cc)::value;
#pragma unroll
                for (int d = 0; d < CB; ++d)
                    acc[c][d] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[c], bv[d], acc[c][d], 0, 0, 0);
                // first half of the stage: up to PPS pieces of the next stage per step, one after each group of CB MFMAs
                constexpr int slot = sidx * PPS + c;
                if constexpr (sidx < STEPS / 2 && c < PPS && slot < NPW) {
                    __builtin_amdgcn_sched_barrier(0);
                    issue(st + NB - 1, bn, slot);
                    __builtin_amdgcn_sched_barrier(0);
                }
            });
            av = av_n;
            bv = bv_n;
        });
        b = b + 1 == NB ? 0 : b + 1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                 // the zero stages issued past the slab's end
    // The k-split waves of a workgroup (KS = 2 or 4 for the narrow tiles) hold partial sums of the SAME tile: they are
    // added here, through the stage buffers, in k order - one record per slab instead of KS (the narrow GEMMs of a
    // NeRF step wrote and re-read 2-4x the partial bytes of the wide ones for a fraction of their work).
    if constexpr (KS > 1) {
        constexpr int WF = gemm_merge_wave_floats(CB);
        __syncthreads();                                             // every wave has left the stage buffers
        if (ks > 0) {
            float* mine = smem + ((ks - 1) * TILES + tile) * WF + lane;
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int d = 0; d < CB; ++d)
#pragma unroll
                    for (int r = 0; r < 16; ++r) mine[((c * CB + d) * 16 + r) * 64] = acc[c][d][r];
#pragma unroll
            for (int q = 0; q < 4; ++q) mine[(4 * CB * 16 + q) * 64] = bsum[q];
        }
        __syncthreads();
        if (ks > 0) return;
#pragma unroll
        for (int k = 1; k < KS; ++k) {
            const float* o = smem + ((k - 1) * TILES + tile) * WF + lane;
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int d = 0; d < CB; ++d)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[c][d][r] += o[((c * CB + d) * 16 + r) * 64];
#pragma unroll
            for (int q = 0; q < 4; ++q) bsum[q] += o[(4 * CB * 16 + q) * 64];
        }
    }
    // write the partial tile: D[row i'][col j] on lane (j, h), reg r: i' = (r&3) + 8*(r>>2) + 4*h
    float* out = partial + (int64_t)blockIdx.x * (TM * TK + (with_bias ? TM : 0));
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ip = (r & 3) + 8 * (r >> 2) + 4 * h;
            bvec v;
#pragma unroll
            for (int d = 0; d < CB; ++d) v[d] = acc[c][d][r];
            *reinterpret_cast<bvec*>(out + (int64_t)(128 * wm + 4 * ip + c) * TK + 32 * CB * wk + CB * i) = v;
        }
    if (with_bias && wk == 0) {
        bsum.x += __shfl_xor(bsum.x, 32); bsum.y += __shfl_xor(bsum.y, 32);
        bsum.z += __shfl_xor(bsum.z, 32); bsum.w += __shfl_xor(bsum.w, 32);
        if (h == 0) *reinterpret_cast<f32x4*>(out + TM * TK + 128 * wm + 4 * i) = bsum;
    }
}

// Thin gradients: out[c][f] = sum_p S[p][c0+c] * H[p][f] for c < nc <= 3, f < F <= 256, plus sum_p S[p][c0+c], plus - in
// the record's fourth row, free once the rows are being read - the column sums sum_p H[p][f] (the bias gradient of a
// layer whose weights are all K = 3 columns).
//   heads:        S = head pre-activation grads [P,4], H = the head's input  -> dW_head[c][f], db_head[c]
//   K = 3 inputs: S = xin [P,8] (xyz | dir),           H = dA of the layer   -> dW[f][col0 + c]
// grid = (point slabs, jobs), block = 256 threads = features; partial[slab][4][256], bias_partial[slab][4] per job.
constexpr int kMaxThinJobs = 6;
struct ThinBatch {
    const float* S[kMaxThinJobs]; const float* H[kMaxThinJobs];
    float* partial[kMaxThinJobs]; float* bias_partial[kMaxThinJobs];
    int lds_[kMaxThinJobs], c0[kMaxThinJobs], nc[kMaxThinJobs], ldh[kMaxThinJobs], F[kMaxThinJobs];
};
template <bool COUNTED = false>
__global__ __launch_bounds__(256) void thin_grad_kernel(ThinBatch tb, std::conditional_t<COUNTED, CountedRows, int64_t> rows_in, int slab_in) {
    int64_t P;
    int slab_pts;
    if constexpr (COUNTED) {                    // as in dw_gemm_kernel; an empty slab's loops do not run: a zero record
        P = counted_rows(rows_in.count, rows_in.capacity);
        slab_pts = counted_slab_pts(P, rows_in.n_slabs);
    } else {
        P = rows_in;
        slab_pts = slab_in;
    }
    const int job = blockIdx.y;
    const float* __restrict__ S = tb.S[job];
    const float* __restrict__ H = tb.H[job];
    float* __restrict__ partial = tb.partial[job];
    float* __restrict__ bias_partial = tb.bias_partial[job];
    const int lds_ = tb.lds_[job], c0 = tb.c0[job], nc = tb.nc[job], ldh = tb.ldh[job], F = tb.F[job];
    // wave w takes points p0 + w, p0 + w + 4, ...; lane l the features 4l..4l+3 (float4 rows, 4 points in flight);
    // the four waves' sums are added in wave order at the end, so the result does not depend on timing
    __shared__ float red[4][4][256];
    __shared__ float bred[4][4];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t p0 = (int64_t)blockIdx.x * slab_pts;
    const int64_t p1 = p0 + slab_pts < P ? p0 + slab_pts : P;
    const bool live = 4 * lane < F;
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0, a3 = a0;
    float b0 = 0.f, b1 = 0.f, b2 = 0.f;
    const auto row = [&](int64_t p) {
        return live ? *reinterpret_cast<const f32x4*>(H + p * ldh + 4 * lane) : f32x4{0.f, 0.f, 0.f, 0.f};
    };
    const auto fma_row = [&](int64_t p, const f32x4& hv) {
        const float* sp = S + p * lds_ + c0;
        const float s0 = sp[0], s1 = nc > 1 ? sp[1] : 0.f, s2 = nc > 2 ? sp[2] : 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            a0[q] = fmaf(s0, hv[q], a0[q]); a1[q] = fmaf(s1, hv[q], a1[q]); a2[q] = fmaf(s2, hv[q], a2[q]);
        }
        a3 += hv;
        b0 += s0; b1 += s1; b2 += s2;
    };
    // eight rows in flight per wave (and four workgroups per CU: BwdBatcher::flush_thin): this kernel is a stream over
    // P x 1 KiB rows, and with four rows per wave and one workgroup per CU only 16 KiB per CU were in flight - 2.9 TB/s
    int64_t p = p0 + w;
    for (; p + 28 < p1; p += 32) {
        const f32x4 h0 = row(p), h1 = row(p + 4), h2 = row(p + 8), h3 = row(p + 12);
        const f32x4 h4 = row(p + 16), h5 = row(p + 20), h6 = row(p + 24), h7 = row(p + 28);
        fma_row(p, h0); fma_row(p + 4, h1); fma_row(p + 8, h2); fma_row(p + 12, h3);
        fma_row(p + 16, h4); fma_row(p + 20, h5); fma_row(p + 24, h6); fma_row(p + 28, h7);
    }
    for (; p < p1; p += 4) fma_row(p, row(p));
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        red[w][0][4 * lane + q] = a0[q]; red[w][1][4 * lane + q] = a1[q]; red[w][2][4 * lane + q] = a2[q];
        red[w][3][4 * lane + q] = a3[q];
    }
    if (lane == 0) { bred[w][0] = b0; bred[w][1] = b1; bred[w][2] = b2; }
    __syncthreads();
    const int f = threadIdx.x;
    float* out = partial + (int64_t)blockIdx.x * 4 * 256;
#pragma unroll
    for (int c = 0; c < 4; ++c) out[c * 256 + f] = ((red[0][c][f] + red[1][c][f]) + red[2][c][f]) + red[3][c][f];
    if (f < 4) {
        float* bo = bias_partial + (int64_t)blockIdx.x * 4;
        bo[f] = f < 3 ? ((bred[0][f] + bred[1][f]) + bred[2][f]) + bred[3][f] : 0.f;
    }
}

// Every cross-slab reduction of a backward pass in ONE launch (grid.y = job), fixed order, deterministic.  A job sums
// n records of `rec` floats element-wise; element idx < TM*TK is tile entry (row, col) = (idx / TK, idx % TK), the
// tail (when bias_dst) the TM bias sums.  Placement: dst[row*ld + col0 + col], or transposed (K = 3 weight columns:
// record [c][f] -> dst[f*ld + col0 + c]).
constexpr int kMaxReduceJobs = 24;
struct ReduceJob {
    const float* src;
    float* dst;
    float* bias_dst;
    int n, rec, TM, TK, ld, col0, rows_valid, cols_valid, transposed;
    int row0 = 0;               // first record row the job places (rows below it belong to another job over the same records)
};
struct ReduceBatch { ReduceJob job[kMaxReduceJobs]; };

__global__ __launch_bounds__(256) void reduce_jobs_kernel(ReduceBatch rb) {
    // Block = 32 float4 entries x 8 k-lanes: lane g sums records g, g+8, g+16, ... (four 16-byte loads in flight), the
    // eight lane sums are added in lane order through LDS - a fixed order whatever the timing.  A job's critical path
    // is n/8 dependent-latency loads instead of n: the 128 x 256 GEMM of a NeRF's dir layer leaves 512 records
    // (256 slabs x 2 k-splits), and with one thread walking all of them the whole launch waited 130 us for it.
    __shared__ f32x4 part[8][32];
    const ReduceJob& j = rb.job[blockIdx.y];
    const int x = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int idx = (blockIdx.x * 32 + x) * 4;
    const bool live = idx < j.rec;
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0, s2 = s0, s3 = s0;
    if (live) {
        const f32x4* p = reinterpret_cast<const f32x4*>(j.src + idx);
        const int64_t stride4 = j.rec / 4;
        int k = g;
        for (; k + 24 < j.n; k += 32) {
            s0 += p[(int64_t)k * stride4]; s1 += p[(int64_t)(k + 8) * stride4];
            s2 += p[(int64_t)(k + 16) * stride4]; s3 += p[(int64_t)(k + 24) * stride4];
        }
        for (; k < j.n; k += 8) s0 += p[(int64_t)k * stride4];
    }
    part[g][x] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (g != 0 || !live) return;
    f32x4 s = part[0][x];
#pragma unroll
    for (int t = 1; t < 8; ++t) s += part[t][x];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = idx + q;
        const bool is_bias = e >= j.TM * j.TK;
        const int row = is_bias ? e - j.TM * j.TK : e / j.TK, col = is_bias ? 0 : e % j.TK;
        if (row >= j.rows_valid || (!is_bias && (col >= j.cols_valid || row < j.row0)) || (is_bias && !j.bias_dst)) continue;
        if (is_bias) j.bias_dst[row] = s[q];
        else if (j.transposed) j.dst[(int64_t)col * j.ld + j.col0 + row] = s[q];
        else j.dst[(int64_t)(row - j.row0) * j.ld + j.col0 + col] = s[q];
    }
}

// ---- host orchestration ---------------------------------------------------------------------
// FiLM scratch: one image's T_l (256x256) and column sums s_l (256) per 256-wide layer, its raw-input columns (256x3, padded)
constexpr int64_t kFilmLayerScratch = 256 * 256 + 256;       // T_l and s_l of one 256-wide FiLM layer
// the L 256-wide FiLM layers of depth L, two K = 3 blocks, s_0 (launch_field_backward)
static int64_t film_partial_floats_depth(int L) { return L * kFilmLayerScratch + 2 * 256 * 4 + 256; }
int64_t film_partial_floats(int64_t /*n_groups*/, int64_t /*points_per_group*/) { return film_partial_floats_depth(8); }
int64_t film_partial_floats_kind(int kind, int64_t /*n_groups*/, int64_t /*points_per_group*/) {
    return is_film(kind) ? film_partial_floats_depth(film_depth(kind)) : 0;
}

static int64_t batched_partial_floats(int kind, int64_t P);
int64_t bwd_partial_floats(int64_t P) {
    // FiLM kinds: one image at a time - eight GEMM jobs of at most 32 slabs each, two thin jobs (or the two head
    // jobs over all images): an upper bound for any image of at most P points.  launch_field_backward checks every
    // pass's real plan against this figure before it launches anything.
    const int64_t slabs256 = (P + 255) / 256 > 0 ? (P + 255) / 256 : 1;          // BwdBatcher::slabs_for never exceeds this
    int64_t most = 8 * (slabs256 < 32 ? slabs256 : 32) * kFilmLayerScratch + 2 * (slabs256 < 512 ? slabs256 : 512) * 1280 + 4096;
    for (int kind = 0; kind < MI_FIELD_KINDS; ++kind) {                           // the others: every job of the pass at once
        if (kFieldKinds[kind].film) continue;
        const int64_t n = batched_partial_floats(kind, P);
        if (n > most) most = n;
    }
    return most;
}
// ... of any kind.  A FiLM image of depth L runs L GEMM jobs of at most ceil(256 / L) slabs each (BwdBatcher::slabs_for):
// 256 job-slabs at depths 4 and 8, but 260 / 258 / 259 at depths 5 / 6 / 7 and up to 264 (depth 12) above 8, so the figure
// above, written for eight jobs of 32 slabs, does not state every depth's plan.  At depths 5 to 7 it is still large enough:
// the extra job-slabs (at most 4 x 65 792 floats) start at 9 217 points, where the NeRF plan in its maximum is already more
// than a million floats above the FiLM term (tests/test_cabi_train_sizes.py replays the planner against this query for
// every depth).  This one is the planner's worst case for the depth itself, never less than the figure above.
int64_t bwd_partial_floats_kind(int kind, int64_t P) {
    const int64_t base = bwd_partial_floats(P);
    const int L = film_depth(kind);
    if (!L) return base;
    const int64_t slabs256 = (P + 255) / 256 > 0 ? (P + 255) / 256 : 1;
    const int64_t cap = (256 + L - 1) / L;
    const int64_t film = L * (slabs256 < cap ? slabs256 : cap) * kFilmLayerScratch + 2 * (slabs256 < 512 ? slabs256 : 512) * 1280 + 4096;
    return film > base ? film : base;
}


// ---- batched orchestration (NeRF, TinyNeRF, SirenNeRF) -----------------------------------------------------------
// A backward pass is: the chain kernel, then every weight-gradient GEMM of one tile shape in ONE launch (grid.y =
// job), the thin (1-/3-row) gradients in one launch, and ONE reduction launch that sums every job's slab partials
// into the gradient tensors - 8 launches for a NeRF (it was 41: at the 1024-ray batch of nerf/train_nerf.py the step
// is launch-bound).  With several jobs per launch a job needs fewer slabs to fill the chip (slabs x jobs ~ 2 per
// CU), so the partial tiles written and re-read shrink by the same factor.
struct BwdBatcher {
    int64_t P;
    float* partial;            // scratch base (null: plan only - used to size the scratch)
    int64_t used = 0;          // floats of scratch handed out
    hipStream_t stream;
    const int* count = nullptr;   // a counted pass: rows [0, *count) of P (the capacity the plan is made from)
    struct Group { GemmBatch b{}; int n = 0; ReduceJob red[kMaxGemmJobs]; } g422, g221, g412, g111;
    ThinBatch thin{};
    int n_thin = 0;
    ReduceJob thin_red[3 * kMaxThinJobs];
    ReduceBatch all{};
    int n_red = 0, max_rec = 0;

    static int slabs_for(int64_t P, int njobs, int per_cu = 1) {
        // one workgroup per CU over the whole launch: the workgroups of a launch do equal work, so a single wave of
        // them has no tail, and fewer slabs mean fewer partial tiles to write and to sum.  (per_cu = 4 for the thin
        // gradients: a 256-thread streaming kernel with no LDS to speak of needs several workgroups per CU to keep
        // enough loads in flight, and its records are 4 KiB, not 256 KiB.)
        int64_t s = (256 * per_cu + njobs - 1) / njobs;
        if (s > 256 * per_cu) s = 256 * per_cu;
        const int64_t most = (P + 255) / 256;              // slabs of at least 256 points
        if (s > most) s = most;
        return (int)(s < 1 ? 1 : s);
    }
    static int slab_pts_for(int64_t P, int slabs) { return (int)(((P + slabs - 1) / slabs + 31) / 32 * 32); }

    float* take(int64_t floats) {
        float* p = partial ? partial + used : nullptr;
        used += (floats + 255) / 256 * 256;
        return p;
    }
    void add_reduce(const ReduceJob& j) {
        all.job[n_red++] = j;
        if (j.rec > max_rec) max_rec = j.rec;
    }
    // dW[M rows][w_ld] at column w_col0 (+ bias gradient gb) = dA^T X over the P points
    template <int CB, int WM, int WK>
    void gemm(Group& g, const float* dA, const float* X, float* gw, int w_ld, int w_col0, int rows_valid, int cols_valid,
              float* gb) {
        constexpr int TM = 128 * WM, TK = 32 * CB * WK;
        g.b.dA[g.n] = dA; g.b.X[g.n] = X; g.b.with_bias[g.n] = gb ? 1 : 0;
        g.red[g.n] = ReduceJob{nullptr, gw, gb, 0, TM * TK + (gb ? TM : 0), TM, TK, w_ld, w_col0, rows_valid, cols_valid, 0};
        ++g.n;
    }
    template <int CB, int WM, int WK>
    int flush(Group& g) {
        if (!g.n) return 0;
        const int slabs = slabs_for(P, g.n), slab = slab_pts_for(P, slabs);
        const int n_slabs = (int)((P + slab - 1) / slab);
        for (int i = 0; i < g.n; ++i) {
            g.red[i].n = n_slabs;                             // one record per slab (k-split waves merge in the kernel)
            g.b.partial[i] = take((int64_t)g.red[i].n * g.red[i].rec);
            g.red[i].src = g.b.partial[i];
            add_reduce(g.red[i]);
        }
        if (!partial) return 0;
        constexpr size_t lds = gemm_lds_bytes<CB, WM, WK>();
        static_assert(lds <= 160 * 1024, "dw_gemm_kernel: this tile shape needs more LDS than a CU has");
        static PerDeviceOnce attr_once;                                               // one per template instance
        const int arc = attr_once.run([&]() {
            for (const void* f : {(const void*)dw_gemm_kernel<CB, WM, WK>, (const void*)dw_gemm_kernel<CB, WM, WK, true>})
                if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
                    set_error("hipFuncSetAttribute(dw_gemm) failed"); return -2;
                }
            return 0;
        });
        if (arc) return arc;
        if (count)
            hipLaunchKernelGGL((dw_gemm_kernel<CB, WM, WK, true>), dim3(n_slabs, g.n), dim3(256), lds, stream, g.b,
                               CountedRows{count, P, n_slabs}, 0);
        else
            hipLaunchKernelGGL((dw_gemm_kernel<CB, WM, WK>), dim3(n_slabs, g.n), dim3(256), lds, stream, g.b, P, slab);
        return check_launch("dw_gemm (batched)");
    }
    // out[c][f] = sum_p S[p][c0+c] H[p][f]: heads (dst [nc][F], bias gb[nc]) or K = 3 weight columns (transposed into
    // dst[f*ld + col0 + c], no bias)
    // colsum_dst: also dst[f] = sum_p H[p][f] (the record's fourth row)
    void thin_job(const float* S, int lds_, int c0, int nc, const float* H, int ldh, int F, float* dst, int ld, int col0,
                  bool transposed, float* gb, float* colsum_dst = nullptr) {
        const int i = n_thin++;
        thin.S[i] = S; thin.lds_[i] = lds_; thin.c0[i] = c0; thin.nc[i] = nc; thin.H[i] = H; thin.ldh[i] = ldh; thin.F[i] = F;
        // record [4][256]: row c, col f
        thin_red[3 * i] = transposed ? ReduceJob{nullptr, dst, nullptr, 0, 1024, 4, 256, ld, col0, nc, F, 1}
                                     : ReduceJob{nullptr, dst, nullptr, 0, 1024, 4, 256, F, 0, nc, F, 0};
        thin_red[3 * i + 1] = gb ? ReduceJob{nullptr, gb, nullptr, 0, 4, 1, 4, 4, 0, 1, nc, 0}
                                 : ReduceJob{nullptr, nullptr, nullptr, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        thin_red[3 * i + 2] = colsum_dst ? ReduceJob{nullptr, colsum_dst, nullptr, 0, 1024, 4, 256, 256, 0, 4, F, 0, 3}
                                         : ReduceJob{nullptr, nullptr, nullptr, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    }
    // The job of one block of a kind's graph (field_kinds.h) into dst[..][ld] at column col0, the bias gradient into
    // bias_dst (null: none).  Engine and tile follow from the block's shape: a head's 1 or 3 rows are a thin job, the 3 raw
    // input columns a transposed one (its bias: the record's column sums), everything else the GEMM of its row widths.
    int add(const GraphBlock& q, float* dst, int ld, int col0, float* bias_dst) {
        if (q.head) thin_job(q.dA, q.da_ld, q.da_c0, q.rows, q.X, q.x_ld, q.cols, dst, ld, col0, false, bias_dst);
        else if (q.cls == SRC_XIN) thin_job(q.X, q.x_ld, q.x_c0, q.cols, q.dA, q.da_ld, q.rows, dst, ld, col0, true, nullptr, bias_dst);
        else if (q.da_ld == 256 && q.x_ld == 256) gemm<4, 2, 2>(g422, q.dA, q.X, dst, ld, col0, q.rows, q.cols, bias_dst);
        else if (q.da_ld == 256 && q.x_ld == 64) gemm<2, 2, 1>(g221, q.dA, q.X, dst, ld, col0, q.rows, q.cols, bias_dst);
        else if (q.da_ld == 128 && q.x_ld == 256) gemm<4, 1, 2>(g412, q.dA, q.X, dst, ld, col0, q.rows, q.cols, bias_dst);
        else if (q.da_ld == 128 && q.x_ld == 32) gemm<1, 1, 1>(g111, q.dA, q.X, dst, ld, col0, q.rows, q.cols, bias_dst);
        else { set_error("no dW engine for a %d x %d block (layer %d)", q.da_ld, q.x_ld, q.layer); return -1; }
        return 0;
    }
    // every launch of the pass: the four GEMM groups, the thin jobs, the reduction
    int flush_all() {
        int rc;
        if ((rc = flush<4, 2, 2>(g422))) return rc;
        if ((rc = flush<2, 2, 1>(g221))) return rc;
        if ((rc = flush<4, 1, 2>(g412))) return rc;
        if ((rc = flush<1, 1, 1>(g111))) return rc;
        if ((rc = flush_thin())) return rc;
        return reduce_all();
    }
    int flush_thin() {
        if (!n_thin) return 0;
        const int slabs = slabs_for(P, n_thin, 4), slab = slab_pts_for(P, slabs);
        const int n_slabs = (int)((P + slab - 1) / slab);
        for (int i = 0; i < n_thin; ++i) {
            thin.partial[i] = take((int64_t)n_slabs * 1024);
            thin.bias_partial[i] = take((int64_t)n_slabs * 4);
            ReduceJob a = thin_red[3 * i], b = thin_red[3 * i + 1], c = thin_red[3 * i + 2];
            a.n = n_slabs; a.src = thin.partial[i];
            add_reduce(a);
            if (b.dst) { b.n = n_slabs; b.src = thin.bias_partial[i]; add_reduce(b); }
            if (c.dst) { c.n = n_slabs; c.src = thin.partial[i]; add_reduce(c); }
        }
        if (!partial) return 0;
        if (count)
            hipLaunchKernelGGL(thin_grad_kernel<true>, dim3(n_slabs, n_thin), dim3(256), 0, stream, thin, CountedRows{count, P, n_slabs}, 0);
        else
            hipLaunchKernelGGL(thin_grad_kernel<false>, dim3(n_slabs, n_thin), dim3(256), 0, stream, thin, P, slab);
        return check_launch("thin_grad (batched)");
    }
    int reduce_all() {
        if (!partial || !n_red) return 0;
        hipLaunchKernelGGL(reduce_jobs_kernel, dim3((max_rec / 4 + 31) / 32, n_red), dim3(256), 0, stream, all);
        return check_launch("reduce_jobs");
    }
};

// The jobs of one backward pass of a non-FiLM kind: every block of its graph into the gradient tensors.  partial == nullptr:
// plan only (b.used = scratch floats needed).
static int batched_backward(int kind, BwdBatcher& b, const float* acts, float* grads, float* const* gp) {
    int rc = 0;
    for_each_block(kFieldKinds[kind], acts, grads, b.P, 0, [&](const GraphBlock& q) {
        if (!rc) rc = b.add(q, gp[2 * q.layer], q.w_ld, q.w_col0, q.bias ? gp[2 * q.layer + 1] : nullptr);
    });
    return rc ? rc : b.flush_all();
}

// A pass's job list is run twice: first as a plan (no scratch, nothing launched) whose scratch need is checked against
// what mi_field_bwd_partial_floats(P) told the caller to allocate - a planning / execution mismatch would otherwise be an
// out-of-bounds write by the GEMMs - then for real over `pts` points.  check = false skips the plan (a pass already
// checked for the same shape).
template <class Jobs>
static int plan_then_run(int kind, int64_t pts, int64_t P, float* partial, hipStream_t stream, const Jobs& jobs, bool check = true,
                         const int* count = nullptr) {
    if (check) {
        BwdBatcher plan{pts, nullptr, 0, stream};
        (void)jobs(plan);
        const int64_t limit = bwd_partial_floats_kind(kind, P);
        if (plan.used > limit) {
            set_error("backward scratch plan (%lld floats) exceeds mi_field_bwd_partial_floats (%lld)", (long long)plan.used,
                      (long long)limit);
            return -1;
        }
    }
    BwdBatcher run{pts, partial, 0, stream, count};
    return jobs(run);
}

// [kind]: the backward chain kernel of each kind
static const void* const kBwdKernels[MI_FIELD_KINDS] = {
    (const void*)nerf_bwd_kernel<false>,      // MI_FIELD_NERF
    (const void*)siren_bwd_kernel<false>,     // MI_FIELD_SIREN_NERF
    (const void*)film_bwd_kernel<true>,       // MI_FIELD_FILM_SIREN_NERF
    (const void*)film_bwd_kernel<false>,      // MI_FIELD_FILM_SIREN_NERF_NODIR
    (const void*)nerf_bwd_kernel<true>};      // MI_FIELD_TINY_NERF
// ... and its counted instance (the kinds an occupancy grid exists for)
static const void* const kCountedBwdKernels[MI_FIELD_KINDS] = {
    (const void*)nerf_bwd_kernel<false, true>, (const void*)siren_bwd_kernel<true>, nullptr, nullptr, (const void*)nerf_bwd_kernel<true, true>};
static_assert(kFilmDepthMax <= kMaxGemmJobs && kFilmDepthMax + 6 <= kMaxReduceJobs,
              "an image's FiLM layers are one GEMM batch and, with the thin jobs, one reduction batch");
// [use_dir]: the run-time-depth FiLM chain (MI_FIELD_FILM_DEPTH kinds other than depth 8)
static const void* const kFilmDepthBwdKernels[2] = {(const void*)film_bwd_kernel<false, true>, (const void*)film_bwd_kernel<true, true>};

// Launches one chain kernel over `blocks` tiles.  The dynamic-LDS attribute of every chain instance is set the first time a
// device is seen; the stamps pointer is the diagnostic build's.  `a` is the kernel's whole argument block: a BwdArgs, or the
// CountedBwdArgs it is the base (and so the first bytes) of.
static int launch_chain(const void* kernel, BwdArgs& a, unsigned blocks, const char* what, hipStream_t stream) {
    const size_t lds = kLdsFloats * sizeof(float);
    static PerDeviceOnce attr_once;
    const int arc = attr_once.run([&]() {
        const struct { const void* const* kernels; int n; } tables[] = {
            {kBwdKernels, MI_FIELD_KINDS}, {kCountedBwdKernels, MI_FIELD_KINDS}, {kFilmDepthBwdKernels, 2}};
        for (const auto& t : tables)
            for (int i = 0; i < t.n; ++i)                // null: a kind without a counted instance
                if (t.kernels[i] && hipFuncSetAttribute(t.kernels[i], hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
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

// Backward of a field over P points.  grad_params[2i], [2i+1]: device pointers to the weight /
// bias gradient tensors (torch layout), overwritten.
int launch_field_backward(int kind_in, const float* packed_bwd, const float* acts, float* grads, const float* raw,
                          const float* g_raw, int64_t n_groups, int64_t points_per_group, const float* film,
                          float* film_partial, float* grad_film, float* partial, float* const* gp,
                          const float* const* params, hipStream_t stream) {
    const int64_t P = n_groups * points_per_group;
    if (P <= 0) return 0;
    if (bad_kind(kind_in)) return -1;
    const int kind = canon_kind(kind_in);
    const bool film_kind = is_film(kind);
    if (film_kind && (!film || !film_partial || !grad_film || !params)) {
        set_error("FiLM backward needs film, the FiLM scratch, grad_film and the parameter pointers");
        return -1;
    }
    const int64_t tpg = (points_per_group + 127) / 128;
    const int L = film_depth(kind);                      // hidden_layers of a FiLM kind: FiLM layers 0..L
    BwdArgs a{packed_bwd, acts, grads, raw, g_raw, P, film, film_partial, points_per_group, tpg, n_groups * tpg, nullptr, L};
    const unsigned blocks = (unsigned)(film_kind ? n_groups * tpg : (P + 127) / 128);
    int rc;
    if ((rc = launch_chain(is_depth_kind(kind) ? kFilmDepthBwdKernels[film_use_dir(kind)] : kBwdKernels[kind], a, blocks,
                           "backward chain", stream))) return rc;
    if (!film_kind)
        return plan_then_run(kind, P, P, partial, stream, [&](BwdBatcher& bb) { return batched_backward(kind, bb, acts, grads, gp); });

    const FieldKind& K = field_kind(kind);
    const int64_t ppg = points_per_group;
    const int n_film = L + 1;                            // rows of an image's FiLM table
    // FiLM scratch of the current image: T_l [256][256] + s_l [256] for the L 256-wide FiLM layers (eight at the reference's
    // depth), the K = 3 blocks of layer 0 (xyz) and of layer L (dir) as [256][3] (padded to 4), s_0 [256]
    const auto Tl = [&](int l) { return film_partial + (int64_t)(l - 1) * kFilmLayerScratch; };
    float* const T3 = film_partial + (int64_t)L * kFilmLayerScratch;
    float* const s0 = T3 + 2 * 256 * 4;
    const auto T = [&](const GraphBlock& q) { return q.cls == SRC_XIN ? T3 + (q.da_region ? 256 * 4 : 0) : Tl(q.da_region); };
    const auto s = [&](const GraphBlock& q) { return q.da_region ? Tl(q.da_region) + 256 * 256 : s0; };
    // Per image g (fixed order, so the sums over images are deterministic): T_g, s_g of every block of a FiLM layer - the
    // 256 x 256 GEMMs of an image are ONE launch (grid.y = layer, a job needs only 32 slabs to give every CU a
    // workgroup, so 8x fewer partial tiles are written and re-read than with a launch per layer), the K = 3 blocks
    // one thin launch, one reduction launch for all of them - then per block (film_finish_kernel)
    // dW += gamma_g (.) T_g, db += gamma_g (.) s_g, d gamma_g = <W, T_g> + b (.) s_g, d beta_g = s_g.
    for (int64_t g = 0; g < n_groups; ++g) {
        const float* frow = film + (g * n_film) * kFilmRow;
        float* dfrow = grad_film + (g * n_film) * kFilmRow;
        const auto jobs = [&](BwdBatcher& bb) -> int {
            int r = 0;
            for_each_block(K, acts, grads, P, g * ppg, [&](const GraphBlock& q) {
                if (!q.head && !r) r = bb.add(q, T(q), q.cols, 0, q.bias ? s(q) : nullptr);
            });
            return r ? r : bb.flush_all();
        };
        if ((rc = plan_then_run(kind, ppg, P, partial, stream, jobs, g == 0))) return rc;   // the plan: first image only
        // a block without the bias part (hidden_layer_rgb's dir columns) is chained behind its layer's job before it
        FinishBatch fb{};
        int n_fin = 0, n_chains = 0;
        fb.first_group = g == 0;
        for_each_block(K, acts, grads, P, g * ppg, [&](const GraphBlock& q) {
            if (q.head) return;
            fb.job[n_fin++] = FinishJob{T(q), s(q), params[2 * q.layer], params[2 * q.layer + 1], frow + q.da_region * kFilmRow,
                                        gp[2 * q.layer], gp[2 * q.layer + 1], dfrow + q.da_region * kFilmRow, q.cols, q.w_ld,
                                        q.w_col0, q.bias};
            n_chains += q.bias;
        });
        hipLaunchKernelGGL(film_finish_kernel, dim3(256, n_chains), dim3(256), 0, stream, fb);
    }
    if ((rc = check_launch("film_finish_kernel"))) return rc;
    // heads: no FiLM in between, all images at once
    return plan_then_run(kind, P, P, partial, stream, [&](BwdBatcher& hb) {
        int r = 0;
        for_each_block(K, acts, grads, P, 0, [&](const GraphBlock& q) {
            if (q.head && !r) r = hb.add(q, gp[2 * q.layer], q.w_ld, q.w_col0, gp[2 * q.layer + 1]);
        });
        return r ? r : hb.flush_all();
    });
}

// Backward of a non-FiLM field over the first *count rows of compact acts (the list-driven training forward left them): the
// counted chain, then the pass's weight-gradient jobs planned from the capacity P and run over the device count.  Every grid
// is sized from P; nothing is read back.
int launch_field_backward_list(int kind_in, const float* packed_bwd, const float* acts, float* grads, const float* raw,
                               const float* g_raw, const int* list, const int* count, int64_t P, float* partial,
                               float* const* gp, hipStream_t stream) {
    if (P <= 0) return 0;
    if (bad_kind(kind_in)) return -1;
    const int kind = canon_kind(kind_in);
    if (kind < 0 || kind >= MI_FIELD_KINDS || !kCountedBwdKernels[kind]) { set_error("kind %d has no counted backward", kind); return -1; }
    CountedBwdArgs a{{packed_bwd, acts, grads, raw, g_raw, P, nullptr, nullptr, P, (P + 127) / 128, (P + 127) / 128, nullptr, 0}, list, count};
    if (const int rc = launch_chain(kCountedBwdKernels[kind], a, (unsigned)((P + 127) / 128), "backward chain (counted)", stream)) return rc;
    return plan_then_run(kind, P, P, partial, stream, [&](BwdBatcher& bb) { return batched_backward(kind, bb, acts, grads, gp); }, true,
                         count);
}

static int64_t batched_partial_floats(int kind, int64_t P) {
    // Plan only (partial == nullptr: nothing is launched, nothing dereferenced).  The gradient pointers must be NON-null
    // here: a job's record is TM*TK floats plus TM bias sums when it has a bias destination, and a plan made with null
    // destinations comes out 256 floats per record short of what the real pass writes.
    static float sink;
    float* gp[2 * kMaxLayers];
    for (float*& g : gp) g = &sink;
    BwdBatcher bb{P, nullptr, 0, nullptr};
    (void)batched_backward(kind, bb, nullptr, nullptr, gp);
    return bb.used + 1024;
}

}  // namespace mi
