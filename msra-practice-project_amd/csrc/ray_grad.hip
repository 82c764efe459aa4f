// ray_grad.hip - dL/d(field inputs) and dL/d(rays) on the fused path (gfx950): what the reference's autograd carries back
// through `network(inputs)` to `pts = o + d z` and `view = d / |d|` (nerf/render.py:93,122,134) - the gradient camera pose
// refinement is built on.  Opt-in: only mirender/pose.py calls these.
//
// The backward chain (field_bwd_chain.hip) has already written dL/d(pre-activation) of every linear layer as
// [point][feature] rows into grads_ws (field_layout.h nerf_grads() .. film_grads_depth()); the gradient of a point's six
// inputs is one more small contraction of the rows of the INPUT-CONSUMING layers with those layers' input columns.  Which
// layers those are, their dA regions, weight columns and saved encoding rows are read from the kind's layer graph
// (field_kinds.h: the blocks whose source is the xin row, E_pos or E_dir); per kind that comes to:
//
//   NeRF / TinyNeRF   dE_pos = dA(layers_pos.0) W0[:, :60] (+ dA(layers_pos.5) W5[:, :60], the skip, nerf/nerf.py:84)
//                     dE_dir = dA(dir layer) Wd[:, 256:280]
//                     then through the encoding E[6i + c] = sin(2^i x_c), E[6i + 3 + c] = cos(2^i x_c) (nerf/nerf.py:44-49):
//                     dx_c = sum_i 2^i (E[6i + 3 + c] dE[6i + c] - E[6i + c] dE[6i + 3 + c])
//   SirenNeRF         dx = dA(layers_pos.0) W0[:, :3] + dA(layers_pos.5) W5[:, :3] (nerf/nerf.py:160),
//                     dv = dA(layers_dir.1) Wd[:, 256:259]
//   FilmSirenNeRF     dx = W_input^T (gamma_0 (.) dL/du_0), dv = W_rgb[:, 256:259]^T (gamma_rgb (.) dL/du_rgb) (use_dir), else 0:
//                     film_bwd_kernel stores dL/du_l = dX_l (.) w_0 cos(w_0 u_l) - the sin derivative is in, gamma is not
//                     (u = gamma (W x + b) + beta, pi_GAN/modules.py:22-25), so gamma multiplies here.
//
// The encoding's sin / cos values are taken from the saved E_pos / E_dir rows (the graph's source regions): the oracle's
// autograd multiplies by cos(2^i x) and sin(2^i x) of the very argument the forward used, the saved rows are the forward's
// values of exactly those (within the forward's own gate), and the point form has no x to recompute them from - acts holds
// the encoding, not the raw input.
//
// Traffic: 1 to 2.5 KiB of dA rows per point (the rows the dW GEMMs also read), next to ~9 KB per point the step already
// moves; the kernels are bound by those reads, not by arithmetic.  Two kernels:
//   input_grad_lin_kernel  (sin kinds, 3 + 3 input columns): a wave takes a point per step, lane l owns features
//                          4l .. 4l + 3 (one coalesced float4 of each dA row), the 3-column weights sit in registers;
//   input_grad_pe_kernel   (ReLU kinds, 60 + 24 encoding columns): lane = encoding column, the weight columns sit in LDS
//                          ([256][64] per position layer, [128][32] for the dir layer), a wave takes four points per step
//                          and reads their dA rows through wave-uniform addresses.
// The ray form gives every ray to ONE wave, which walks the ray's samples in order, keeps per-lane partial sums and
// reduces across lanes once per ray: g_o = sum_s g_pos, g_d = sum_s z_s g_pos + (I - v v^T) / |d| sum_s g_dir (v = d / |d|).
// Lanes 0..5 of that wave write the ray's six floats in one store instruction; no atomics, so a result does not depend
// on the launch's timing.
// The LIST instances of the two ray-form kernels (training with an occupancy grid) read COMPACT dA / E rows
// through the ascending list of a counted backward (launch_field_backward_list): ray r's samples are the run [e0, e1) of the
// list with r S <= list[e] < (r + 1) S, found by two wave-uniform binary searches of the device-counted list; entry e reads row
// e of every region, z[list[e]] and the ray's own six floats.  An unlisted sample's raw is the constant 0 and sends the rays
// nothing: the run is all a ray has.  Same per-point arithmetic, same order along the ray, same store_ray.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "field_kinds_host.h"
#include "launchers.h"

namespace mi {

struct InputGradArgs {
    const float* dA0; const float* dA5; const float* dAd;     // dA rows of the consuming layers: [P][256] x2, [P][dir_rows]
    const float* W0; const float* W5; const float* Wd;        // their weights [out][ld]; W5 / Wd null: the kind has none
    int ld0, ld5, ldd;
    int col_d;                 // first view-direction (encoding) column of Wd
    int dir_rows;              // output features of the dir-consuming layer: 128, or 256 (FiLM)
    const float* film;         // FiLM kinds: [groups][film_rows][512], else null
    int film_rows, film_dir_row;
    const float* e_pos; const float* e_dir;                   // ReLU kinds: saved encoding rows [P][64], [P][32]
    const float* rays; const float* z;                        // ray form: [n,2,3], [n,S]
    float* out;                // point form: g_x [P,6]; ray form: g_rays [n,2,3]
    int64_t units;             // ray form: rays; point form: chunks of kChunk points that do not straddle a group
    int64_t units_per_group;
    int64_t points_per_group;
    int n_samples;
    int accumulate;
};

// ... and of the list form: rows are entries of `list` (ascending point indices, *count of them, read on the device)
struct InputGradListArgs : InputGradArgs {
    const int* list; const int* count;
    int capacity;              // n * n_samples: no more entries than that, whatever *count holds
};
template <bool LIST>
using InputGradArgsOf = std::conditional_t<LIST, InputGradListArgs, InputGradArgs>;

constexpr int kChunk = 32;     // points of a point-form unit

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// first point and point count of unit u (wave-uniform), and its FiLM group
template <bool RAYS>
__device__ __forceinline__ void unit_points(const InputGradArgs& a, int64_t u, int64_t& p0, int& cnt, int64_t& group) {
    group = u / a.units_per_group;
    if constexpr (RAYS) {
        p0 = u * a.n_samples;
        cnt = a.n_samples;
    } else {
        const int64_t c = u % a.units_per_group;
        p0 = group * a.points_per_group + c * kChunk;
        const int64_t left = a.points_per_group - c * kChunk;
        cnt = left < kChunk ? (int)left : kChunk;
    }
}

// first entry of list[lo .. hi) that is >= key, hi if none (wave-uniform: the loads are scalar, the list sits in L2)
__device__ __forceinline__ int list_lower_bound(const int* list, int lo, int hi, int64_t key) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (list[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ... and of ray u of the list form: its run of entries [p0, p0 + cnt) - rows of the compact regions; cnt = 0: none listed.
// The second search starts at the first one's result and ends n_samples entries on at the latest.
__device__ __forceinline__ void unit_entries(const InputGradListArgs& a, int64_t u, int64_t& p0, int& cnt) {
    int count = *a.count;
    count = count < 0 ? 0 : count > a.capacity ? a.capacity : count;
    const int e0 = list_lower_bound(a.list, 0, count, u * a.n_samples);
    const int end = count - e0 < a.n_samples ? count : e0 + a.n_samples;
    p0 = e0;
    cnt = list_lower_bound(a.list, e0, end, (u + 1) * a.n_samples) - e0;
}

// Lanes 0..5 write a ray's (g_o | g_d) from the ray's reduced sums (every lane holds them): so = sum g_pos,
// sz = sum z g_pos, sv = sum g_dir.
__device__ __forceinline__ void store_ray(const InputGradArgs& a, int64_t ray, int lane, const float (&so)[3],
                                          const float (&sz)[3], const float (&sv)[3]) {
    const float* d = a.rays + ray * 6 + 3;
    const float d0 = d[0], d1 = d[1], d2 = d[2];
    const float nrm = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
    const float v0 = d0 / nrm, v1 = d1 / nrm, v2 = d2 / nrm;
    const float vg = v0 * sv[0] + v1 * sv[1] + v2 * sv[2];
    const float g[6] = {so[0], so[1], so[2], sz[0] + (sv[0] - v0 * vg) / nrm, sz[1] + (sv[1] - v1 * vg) / nrm,
                        sz[2] + (sv[2] - v2 * vg) / nrm};
    float mine = g[0];
#pragma unroll
    for (int j = 1; j < 6; ++j) mine = lane == j ? g[j] : mine;
    if (lane < 6) {
        float* o = a.out + ray * 6 + lane;
        *o = a.accumulate ? *o + mine : mine;
    }
}

// =========================================================================================
// sin kinds: raw xyz / dir inputs, three columns per consuming layer
// =========================================================================================
template <bool RAYS, bool LIST = false>
__global__ __launch_bounds__(256) void input_grad_lin_kernel(InputGradArgsOf<LIST> a) {
    static_assert(RAYS || !LIST, "the list form is a ray form");
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool dir_lane = a.Wd && 4 * lane < a.dir_rows;
    float w0[4][3], w5[4][3], wd[4][3];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int k = 4 * lane + q;
            w0[q][j] = a.W0[(int64_t)k * a.ld0 + j];
            w5[q][j] = a.W5 ? a.W5[(int64_t)k * a.ld5 + j] : 0.f;
            wd[q][j] = dir_lane ? a.Wd[(int64_t)k * a.ldd + a.col_d + j] : 0.f;
        }
    const int64_t stride = (int64_t)gridDim.x * 4;
    for (int64_t u = (int64_t)blockIdx.x * 4 + wave; u < a.units; u += stride) {
        int64_t p0, group = 0;
        int cnt;
        if constexpr (LIST) unit_entries(a, u, p0, cnt);
        else unit_points<RAYS>(a, u, p0, cnt, group);
        float4 g0 = {1.f, 1.f, 1.f, 1.f}, gd = {1.f, 1.f, 1.f, 1.f};
        if (a.film) {                                     // gamma of the input layer and of the rgb hidden layer
            const float* row = a.film + group * ((int64_t)a.film_rows * kFilmRow);
            g0 = reinterpret_cast<const float4*>(row)[lane];
            gd = reinterpret_cast<const float4*>(row + (int64_t)a.film_dir_row * kFilmRow)[lane];
        }
        float so[3] = {0.f, 0.f, 0.f}, sz[3] = {0.f, 0.f, 0.f}, sv[3] = {0.f, 0.f, 0.f};
        for (int s = 0; s < cnt; ++s) {
            const int64_t p = p0 + s;
            float4 r = reinterpret_cast<const float4*>(a.dA0 + p * 256)[lane];
            r.x *= g0.x; r.y *= g0.y; r.z *= g0.z; r.w *= g0.w;
            float gp[3], gv[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) gp[j] = r.x * w0[0][j] + r.y * w0[1][j] + r.z * w0[2][j] + r.w * w0[3][j];
            if (a.dA5) {
                const float4 t = reinterpret_cast<const float4*>(a.dA5 + p * 256)[lane];
#pragma unroll
                for (int j = 0; j < 3; ++j) gp[j] += t.x * w5[0][j] + t.y * w5[1][j] + t.z * w5[2][j] + t.w * w5[3][j];
            }
            float4 t = {0.f, 0.f, 0.f, 0.f};
            if (dir_lane) t = reinterpret_cast<const float4*>(a.dAd + p * a.dir_rows)[lane];
            t.x *= gd.x; t.y *= gd.y; t.z *= gd.z; t.w *= gd.w;
#pragma unroll
            for (int j = 0; j < 3; ++j) gv[j] = t.x * wd[0][j] + t.y * wd[1][j] + t.z * wd[2][j] + t.w * wd[3][j];
            if constexpr (RAYS) {
                float zs;
                if constexpr (LIST) zs = a.z[a.list[p]];                // p is the row; the depth is the point's
                else zs = a.z[p];
#pragma unroll
                for (int j = 0; j < 3; ++j) { so[j] += gp[j]; sz[j] += zs * gp[j]; sv[j] += gv[j]; }
            } else {
                float mine = 0.f;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const float x = wave_sum(gp[j]), v = wave_sum(gv[j]);
                    mine = lane == j ? x : lane == 3 + j ? v : mine;
                }
                if (lane < 6) a.out[p * 6 + lane] = mine;
            }
        }
        if constexpr (RAYS) {
#pragma unroll
            for (int j = 0; j < 3; ++j) { so[j] = wave_sum(so[j]); sz[j] = wave_sum(sz[j]); sv[j] = wave_sum(sv[j]); }
            store_ray(a, u, lane, so, sz, sv);
        }
    }
}

// =========================================================================================
// ReLU kinds: positional encodings, 60 + 24 columns
// =========================================================================================
constexpr int kPeThreads = 1024;                  // 16 waves share one copy of the weight columns in LDS
constexpr int kPePosFloats = 256 * 64, kPeDirFloats = 128 * 32;

// dE[q] += sum_k rows[q][k] * cols[k][lane]: rows through wave-uniform addresses, columns from LDS
template <int K, int LDW>
__device__ __forceinline__ void pe_contract(float (&dE)[4], const float* const (&rows)[4], const float* cols, int col) {
#pragma unroll 2
    for (int k = 0; k < K; k += 4) {
        float w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = cols[(k + i) * LDW + col];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 r = *reinterpret_cast<const float4*>(rows[q] + k);
            dE[q] = fmaf(r.x, w[0], dE[q]);
            dE[q] = fmaf(r.y, w[1], dE[q]);
            dE[q] = fmaf(r.z, w[2], dE[q]);
            dE[q] = fmaf(r.w, w[3], dE[q]);
        }
    }
}

// A listed point's terms added to the per-lane sums of its ray with the roundings of the plain ray form, whose compiled code
// is the contract (tools/isa_diff.py holds it; tests/test_gpu_occupancy_pose.py holds this to it bit for bit).  There the
// compiler fused the multiply into the add for the FIRST point of every 4-point step - tz = fma(z, t, tz) and
// tv = fma(coef_d, dE_d e_d, tv) - and for the other three it adds the rounded products; tp takes the rounded t always.  The plain
// form's steps start at the samples s = 0, 4, 8 .. of the ray, the list form's at every fourth ENTRY of the run: `lead` says
// whether this point's sample index is a multiple of 4, so a listed sample is rounded as the plain form rounds it, wherever it
// falls in the run.  Nothing here may be contracted further, hence the pragma; the two fused terms are spelled fmaf.
__device__ __forceinline__ void add_as_plain_step(bool lead, float dEp, float ep, float coef_p, float dEd, float ed, float coef_d,
                                                  float zs, float& tp, float& tz, float& tv) {
#pragma clang fp contract(off)
    const float t = (dEp * ep) * coef_p;
    const float pd = dEd * ed;
    tp = tp + t;
    if (lead) {
        tz = fmaf(zs, t, tz);
        tv = fmaf(coef_d, pd, tv);
    } else {
        const float zt = zs * t, v = pd * coef_d;
        tz = tz + zt;
        tv = tv + v;
    }
}

template <bool RAYS, bool LIST = false>
__global__ __launch_bounds__(kPeThreads) void input_grad_pe_kernel(InputGradArgsOf<LIST> a) {
    static_assert(RAYS || !LIST, "the list form is a ray form");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* L0 = lds;
    float* L5 = lds + kPePosFloats;
    float* Ld = lds + (a.W5 ? 2 : 1) * kPePosFloats;
    for (int i = threadIdx.x; i < kPePosFloats; i += kPeThreads) {
        const int k = i >> 6, c = i & 63;
        L0[i] = c < 60 ? a.W0[(int64_t)k * a.ld0 + c] : 0.f;
        if (a.W5) L5[i] = c < 60 ? a.W5[(int64_t)k * a.ld5 + c] : 0.f;
    }
    for (int i = threadIdx.x; i < kPeDirFloats; i += kPeThreads) {
        const int k = i >> 5, c = i & 31;
        Ld[i] = c < 24 ? a.Wd[(int64_t)k * a.ldd + a.col_d + c] : 0.f;
    }
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // lane f <-> encoding feature f = 6 i + c: c < 3 sin(2^i x_c), else cos(2^i x_{c-3}); its partner holds the other one.
    // d sin(s x) = s cos(s x) dx, d cos(s x) = -s sin(s x) dx: coef = +-2^i times the partner's saved value.
    const int fi = lane / 6, fc = lane % 6;
    const bool is_cos = fc >= 3;
    const int comp = fc % 3;
    const int mate_p = lane < 60 ? (is_cos ? lane - 3 : lane + 3) : lane;
    const float coef_p = lane < 60 ? (is_cos ? -(float)(1 << fi) : (float)(1 << fi)) : 0.f;
    const int dl = lane & 31;
    // lanes < 24: same (i, c) as above.  The others carry no direction column (coef_d = 0) and read column dl of the point's
    // OWN row - 0 * NaN is NaN, so a zero coefficient does not excuse a read outside what the forward wrote for this point
    const int mate_d = lane < 24 ? (is_cos ? lane - 3 : lane + 3) : dl;
    const float coef_d = lane < 24 ? (is_cos ? -(float)(1 << fi) : (float)(1 << fi)) : 0.f;

    const int64_t stride = (int64_t)gridDim.x * (kPeThreads / 64);
    for (int64_t u = (int64_t)blockIdx.x * (kPeThreads / 64) + wave; u < a.units; u += stride) {
        int64_t p0, group = 0;
        int cnt;
        if constexpr (LIST) unit_entries(a, u, p0, cnt);
        else unit_points<RAYS>(a, u, p0, cnt, group);
        float tp = 0.f, tz = 0.f, tv = 0.f;                // ray form: per-lane sums over the ray's samples
        for (int s0 = 0; s0 < cnt; s0 += 4) {
            int64_t p[4];
            const float* r0[4];
            const float* r5[4];
            const float* rd[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                p[q] = p0 + (s0 + q < cnt ? s0 + q : cnt - 1);           // past the unit's end: its last point again, masked below
                r0[q] = a.dA0 + p[q] * 256;
                r5[q] = a.dA5 ? a.dA5 + p[q] * 256 : nullptr;
                rd[q] = a.dAd + p[q] * 128;
            }
            float dEp[4] = {0.f, 0.f, 0.f, 0.f}, dEd[4] = {0.f, 0.f, 0.f, 0.f};
            pe_contract<256, 64>(dEp, r0, L0, lane);
            if (a.W5) pe_contract<256, 64>(dEp, r5, L5, lane);
            pe_contract<128, 32>(dEd, rd, Ld, dl);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bool in = s0 + q < cnt;
                const float ep = a.e_pos[p[q] * 64 + mate_p], ed = a.e_dir[p[q] * 32 + mate_d];
                const float t = in ? (dEp[q] * ep) * coef_p : 0.f;
                const float v = in ? (dEd[q] * ed) * coef_d : 0.f;
                if constexpr (LIST) {
                    if (in) {                                           // wave-uniform; p[q] is the row, the depth is the point's
                        const int pt = a.list[p[q]];
                        add_as_plain_step(((pt - (int)u * a.n_samples) & 3) == 0, dEp[q], ep, coef_p, dEd[q], ed, coef_d, a.z[pt], tp,
                                          tz, tv);
                    }
                } else if constexpr (RAYS) {
                    const float zs = a.z[p[q]];
                    tp += t; tz += zs * t; tv += v;
                } else if (in) {                                        // wave-uniform
                    float mine = 0.f;
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const float x = wave_sum(comp == j ? t : 0.f), w = wave_sum(comp == j ? v : 0.f);
                        mine = lane == j ? x : lane == 3 + j ? w : mine;
                    }
                    if (lane < 6) a.out[p[q] * 6 + lane] = mine;
                }
            }
        }
        if constexpr (RAYS) {
            float so[3], sz[3], sv[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                so[j] = wave_sum(comp == j ? tp : 0.f);
                sz[j] = wave_sum(comp == j ? tz : 0.f);
                sv[j] = wave_sum(comp == j ? tv : 0.f);
            }
            store_ray(a, u, lane, so, sz, sv);
        }
    }
}

// =========================================================================================
// host side
// =========================================================================================
static int launch_input_grad(int kind_in, const float* const* params, const float* film, const float* acts,
                             const float* grads, const float* rays, const float* z, int64_t n_groups, int64_t units_pg,
                             int n_samples, bool ray_form, int accumulate, float* out, hipStream_t stream,
                             const int* list = nullptr, const int* count = nullptr) {
    const int kind = canon_kind(kind_in);
    const FieldKind& K = field_kind(kind);
    const int64_t ppg = ray_form ? units_pg * n_samples : units_pg;
    const int64_t P = n_groups * ppg;
    if (P == 0) return 0;
    InputGradListArgs a = {};                           // the plain forms take its base
    a.list = list; a.count = count; a.capacity = (int)P;    // list form: P = n * S fits an int (the caller checks)
    a.rays = rays; a.z = z; a.out = out; a.n_samples = n_samples; a.accumulate = accumulate;
    a.points_per_group = ppg;
    a.units_per_group = ray_form ? units_pg : (ppg + kChunk - 1) / kChunk;
    a.units = n_groups * a.units_per_group;
    if (K.film) { a.film = film; a.film_rows = film_layers(kind); a.film_dir_row = a.film_rows - 1; }   // gamma rows: read even
    bool pe = false;                                                                    // where no layer reads the direction
    // the blocks of the kind's graph (field_kinds.h) that read the raw input or its encoding: first and second position
    // consumer, then the direction consumer (graph_ok: a kind has no more)
    for_each_block(K, acts, grads, P, 0, [&](const GraphBlock& q) {
        const float* W = params[2 * q.layer];
        if (q.cls == SRC_E_POS || (q.cls == SRC_XIN && q.x_c0 == 0)) {
            if (!a.W0) { a.W0 = W; a.ld0 = q.w_ld; a.dA0 = q.dA; }
            else { a.W5 = W; a.ld5 = q.w_ld; a.dA5 = q.dA; }
            if (q.cls == SRC_E_POS) { pe = true; a.e_pos = q.X; }
        } else if (q.cls != SRC_HIDDEN) {
            a.Wd = W; a.ldd = q.w_ld; a.dAd = q.dA; a.col_d = q.w_col0; a.dir_rows = q.rows;
            if (K.film) a.film_dir_row = q.da_region;
            if (q.cls == SRC_E_DIR) a.e_dir = q.X;
        }
    });
    const InputGradArgs& plain = a;
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (pe) {
        const size_t lds = ((a.W5 ? 2 : 1) * kPePosFloats + kPeDirFloats) * sizeof(float);
        static_assert((2 * kPePosFloats + kPeDirFloats) * sizeof(float) <= 160 * 1024, "the weight columns fit a CU's LDS");
        const void* fn = list ? (const void*)input_grad_pe_kernel<true, true>
                         : ray_form ? (const void*)input_grad_pe_kernel<true> : (const void*)input_grad_pe_kernel<false>;
        static PerDeviceOnce attr_once[3];
        const int arc = attr_once[list ? 2 : ray_form].run([&]() {
            if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)((2 * kPePosFloats + kPeDirFloats) * sizeof(float))) != hipSuccess) {
                set_error("hipFuncSetAttribute(input_grad_pe) failed"); return -2;
            }
            return 0;
        });
        if (arc) return arc;
        const int64_t per_block = kPeThreads / 64;
        const int64_t want = (a.units + per_block - 1) / per_block;
        const dim3 grid((unsigned)(want < cus ? want : cus));
        if (list) hipLaunchKernelGGL((input_grad_pe_kernel<true, true>), grid, dim3(kPeThreads), lds, stream, a);
        else if (ray_form) hipLaunchKernelGGL(input_grad_pe_kernel<true>, grid, dim3(kPeThreads), lds, stream, plain);
        else hipLaunchKernelGGL(input_grad_pe_kernel<false>, grid, dim3(kPeThreads), lds, stream, plain);
        return check_launch("input_grad_pe");
    }
    const int64_t want = (a.units + 3) / 4, cap = (int64_t)cus * 8;
    const dim3 grid((unsigned)(want < cap ? want : cap));
    if (list) hipLaunchKernelGGL((input_grad_lin_kernel<true, true>), grid, dim3(256), 0, stream, a);
    else if (ray_form) hipLaunchKernelGGL(input_grad_lin_kernel<true>, grid, dim3(256), 0, stream, plain);
    else hipLaunchKernelGGL(input_grad_lin_kernel<false>, grid, dim3(256), 0, stream, plain);
    return check_launch("input_grad_lin");
}

int launch_field_input_grad(int kind, const float* const* params, const float* film, const float* acts, const float* grads,
                            int64_t n_groups, int64_t points_per_group, float* g_x, hipStream_t stream) {
    return launch_input_grad(kind, params, film, acts, grads, nullptr, nullptr, n_groups, points_per_group, 1, false, 0,
                             g_x, stream);
}

int launch_field_input_grad_rays(int kind, const float* const* params, const float* film, const float* acts,
                                 const float* grads, const float* rays, const float* z, int64_t n_groups,
                                 int64_t rays_per_group, int n_samples, int accumulate, float* g_rays, hipStream_t stream) {
    return launch_input_grad(kind, params, film, acts, grads, rays, z, n_groups, rays_per_group, n_samples, true, accumulate,
                             g_rays, stream);
}

int launch_field_input_grad_rays_list(int kind, const float* const* params, const float* acts, const float* grads,
                                      const int* list, const int* count, const float* rays, const float* z, int64_t n,
                                      int n_samples, int accumulate, float* g_rays, hipStream_t stream) {
    return launch_input_grad(kind, params, nullptr, acts, grads, rays, z, 1, n, n_samples, true, accumulate, g_rays, stream,
                             list, count);
}

}  // namespace mi
