// train_path.hip - one training step of render_rays through the C ABI (include/mi_render.h): mi_render_rays_train
// (the forward, which keeps layer inputs) and mi_render_rays_backward (every parameter gradient and the FiLM-table
// gradient from the six output cotangents), plus their size queries and mi::grad_accumulate_kernel.
//
// This is the host orchestration of mirender/autograd.py (_RenderRaysFn, _forward_pass, _field_backward,
// _chunk_ranges) restated without torch.  Both copies must give the same bits; tests/test_gpu_cabi_train.py holds them
// to it.  What has to match, decision by decision:
//   - ray ranges: a pass of S samples per ray is cut into ranges of at most range_points / S rays (whole FiLM groups
//     per range, or equal parts of one group when one image alone is larger: _chunk_ranges);
//   - kept layer inputs: the forward fills `saved` with the inputs of the leading ranges of the coarse pass, then of
//     the second pass, stopping in each pass at the first range that does not fit; the backward derives the same plan
//     and recomputes every other range (bit-identical, tests/test_gpu_train.py);
//   - sums, in autograd's order: the first range of a pass writes the pass's gradients, each later range goes to
//     scratch and is added; one field: the coarse-point total, then += the new-sample total; grad_film = coarse pass +
//     fine pass; Nf = 0 with one field: g_raw = coarse + fine before one field backward.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "render_path.h"

namespace mi {

// ---- grad_accumulate_kernel: dst[i] += src[i] over a table of tensors, one launch --------------------------------
// What torch._foreach_add_ / `+=` do for autograd (fp32, one rounding per element, so the same bits).  HBM-bound: each
// lane moves one float4 of dst and src per iteration when both pointers are 16-byte aligned (a wave64 covers 1 KiB),
// the scalar tail / unaligned tensors go one float per lane.  grid: (blocks per tensor, entries); block 256.
constexpr int kAccMaxEntries = 2 * kMaxLayers + 1;       // one field's parameters + one FiLM row / table

struct AccTable {
    float* dst[kAccMaxEntries];
    const float* src[kAccMaxEntries];
    int64_t numel[kAccMaxEntries];
    int vec4[kAccMaxEntries];
};

__global__ __launch_bounds__(256) void grad_accumulate_kernel(AccTable t) {
    const int e = blockIdx.y;
    float* __restrict__ d = t.dst[e];
    const float* __restrict__ s = t.src[e];
    const int64_t n = t.numel[e];
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t head = 0;
    if (t.vec4[e]) {
        const int64_t n4 = n >> 2;
        float4* __restrict__ d4 = reinterpret_cast<float4*>(d);
        const float4* __restrict__ s4 = reinterpret_cast<const float4*>(s);
        for (int64_t j = i0; j < n4; j += stride) {
            float4 a = d4[j];
            const float4 b = s4[j];
            a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
            d4[j] = a;
        }
        head = n4 << 2;
    }
    for (int64_t j = head + i0; j < n; j += stride) d[j] += s[j];
}

// Host side: collects (dst, src, numel) entries and launches once per kAccMaxEntries.
struct Accumulator {
    AccTable t{};
    int n = 0;
    int64_t most = 0;
    hipStream_t stream;
    explicit Accumulator(hipStream_t s) : stream(s) {}
    int add(float* dst, const float* src, int64_t numel) {
        if (numel <= 0) return MI_OK;
        if (n == kAccMaxEntries)
            if (int rc = flush()) return rc;
        t.dst[n] = dst; t.src[n] = src; t.numel[n] = numel;
        t.vec4[n] = ((uintptr_t)dst % 16 == 0) && ((uintptr_t)src % 16 == 0);
        const int64_t work = t.vec4[n] ? (numel + 3) / 4 : numel;
        if (work > most) most = work;
        ++n;
        return MI_OK;
    }
    int flush() {
        if (n == 0) return MI_OK;
        const int64_t bx = (most + 255) / 256 < 128 ? (most + 255) / 256 : 128;
        hipLaunchKernelGGL(grad_accumulate_kernel, dim3((unsigned)bx, n), dim3(256), 0, stream, t);
        n = 0; most = 0;
        return check_launch("grad_accumulate_kernel");
    }
};

// ---- ray ranges (autograd._chunk_ranges) --------------------------------------------------------------------------
struct Ranges {
    bool film = false, parts = false;
    int64_t n = 0, groups = 1, rpg = 0, step = 1, per_group = 1;
    int S = 1;
    int64_t count() const { return parts ? groups * per_group : (n + step - 1) / step; }
    void get(int64_t k, int64_t& r0, int64_t& r1) const {
        if (!parts) { r0 = k * step; r1 = r0 + step < n ? r0 + step : n; return; }
        const int64_t g = k / per_group, a = (k % per_group) * step;
        r0 = g * rpg + a;
        r1 = g * rpg + (a + step < rpg ? a + step : rpg);
    }
};

static Ranges make_ranges(int kind, int64_t n_groups, int64_t rays_per_group, int S, int64_t range_points) {
    Ranges R;
    R.film = is_film(kind);
    R.n = n_groups * rays_per_group;
    R.S = S;
    R.groups = R.film ? n_groups : 1;
    R.rpg = R.film ? rays_per_group : R.n;
    const int64_t max_rays = range_points / S > 1 ? range_points / S : 1;
    if (!R.film || max_rays >= R.rpg) {
        R.step = R.film ? (max_rays / R.rpg) * R.rpg : max_rays;       // whole FiLM groups per range
    } else {                                                         // one image exceeds a range: equal parts of it
        const int64_t parts = (R.rpg + max_rays - 1) / max_rays;
        R.parts = true;
        R.step = (R.rpg + parts - 1) / parts;
        R.per_group = (R.rpg + R.step - 1) / R.step;
    }
    return R;
}

// FiLM rows of a range: its whole groups, or the one group it is a part of (autograd._film_of_range)
static void range_groups(const Ranges& R, int64_t r0, int64_t r1, int64_t& g0, int64_t& ng) {
    if (!R.film) { g0 = 0; ng = 1; return; }
    g0 = r0 / R.rpg;
    ng = r1 / R.rpg > g0 + 1 ? r1 / R.rpg - g0 : 1;
}

// ---- the two passes of one call ------------------------------------------------------------------------------------
struct PassSpec {
    bool exists;
    int kind;
    int S;
    int64_t range_points;
};

// pass 0 = coarse (Nc samples); pass 1 = fine over Nc + Nf (two fields), the Nf new depths (one field), none (one
// field with Nf = 0: the fine pass is the coarse pass)
static void pass_specs(int kind_c, int kind_f, const RenderCall& G, int64_t rp_c, int64_t rp_f, PassSpec P[2]) {
    P[0] = {true, kind_c, G.Nc, rp_c};
    if (!G.shared) P[1] = {true, kind_f, G.Nc + G.Nf, rp_f};
    else P[1] = {G.Nf > 0, kind_c, G.Nf, rp_f};
}

// How many leading ranges of each pass keep their layer inputs within saved_bytes (autograd._forward_pass's loop,
// coarse pass first, one budget).  Returns the floats the coarse pass keeps: the second pass's kept inputs follow them.
static int64_t plan_kept(const PassSpec P[2], const RenderCall& G, int64_t saved_bytes, int64_t kept[2]) {
    int64_t budget = saved_bytes, coarse_floats = 0;
    for (int p = 0; p < 2; ++p) {
        kept[p] = 0;
        if (!P[p].exists) continue;
        const Ranges R = make_ranges(P[p].kind, G.n_groups, G.rays_per_group, P[p].S, P[p].range_points);
        const int64_t per_ray = 4 * region_total(field_kind(P[p].kind).acts) * (int64_t)P[p].S;
        for (int64_t k = 0, c = R.count(); k < c; ++k) {
            int64_t r0, r1;
            R.get(k, r0, r1);
            const int64_t need = per_ray * (r1 - r0);
            if (need > budget) break;
            budget -= need;
            ++kept[p];
        }
        if (p == 0) coarse_floats = (saved_bytes - budget) / 4;
    }
    return coarse_floats;
}

static int64_t param_numel(int kind, int i) {
    const FieldKind& k = field_kind(kind);
    return (i & 1) ? k.dims[i / 2][0] : (int64_t)k.dims[i / 2][0] * k.dims[i / 2][1];
}

// a scratch copy of a kind's parameter gradients: tensor after tensor, each starting on a 64-float block
int64_t param_floats(int kind) {
    int64_t f = 0;
    for (int i = 0; i < 2 * field_kind(kind).n_layers; ++i) f += align64(param_numel(kind, i));
    return f;
}

// Regions of the backward workspace, in floats, each 64-float (256-byte) aligned.
struct BwdLayout {
    int64_t g_raw_c, g_raw_f, g_raw_s;             // dL/d(raw) of the coarse / fine composite, of the new samples
    int64_t range_params, fine_total;              // a later range's parameter gradients; one field: the new-sample total
    int64_t film_pass, film_row;                   // the second FiLM pass's table gradient; a later part's row
    int64_t acts, raw, grads, partial, film_partial;   // one range: recomputed inputs and raw, dA, dW and FiLM scratch
    int64_t total;
};

static BwdLayout bwd_layout(const PassSpec P[2], const RenderCall& G) {
    int64_t sz_acts = 0, sz_raw = 0, sz_grads = 0, sz_part = 0, sz_fpart = 0, sz_params = 0;
    bool any_film = false;
    int64_t film_fl = 0;                           // one group's rows of the FiLM table (two FiLM fields: the same depth)
    for (int p = 0; p < 2; ++p) {
        if (!P[p].exists) continue;
        if (film_floats(P[p].kind) > film_fl) film_fl = film_floats(P[p].kind);
        const FieldKind& K = field_kind(P[p].kind);
        const Ranges R = make_ranges(P[p].kind, G.n_groups, G.rays_per_group, P[p].S, P[p].range_points);
        // every range has the shape of the first, the last, or (parts of images) the last part of an image
        const int64_t probes[3] = {0, R.count() - 1, R.parts ? R.per_group - 1 : 0};
        for (int64_t k : probes) {
            int64_t r0, r1, g0, ng;
            R.get(k, r0, r1);
            range_groups(R, r0, r1, g0, ng);
            const int64_t pts = (r1 - r0) * P[p].S;
            sz_acts = pts * region_total(K.acts) > sz_acts ? pts * region_total(K.acts) : sz_acts;
            sz_raw = pts * 4 > sz_raw ? pts * 4 : sz_raw;
            sz_grads = pts * region_total(K.grads) > sz_grads ? pts * region_total(K.grads) : sz_grads;
            const int64_t bp = bwd_partial_floats_kind(P[p].kind, pts);
            sz_part = bp > sz_part ? bp : sz_part;
            if (R.film) {
                const int64_t fp = film_partial_floats_kind(P[p].kind, ng, pts / ng);
                sz_fpart = fp > sz_fpart ? fp : sz_fpart;
            }
        }
        any_film |= R.film;
        sz_params = param_floats(P[p].kind) > sz_params ? param_floats(P[p].kind) : sz_params;
    }
    BwdLayout L{};
    RegionAllocator ws;
    const int64_t n = G.n;
    L.g_raw_c = ws.take(n * G.Nc * 4);
    L.g_raw_f = ws.take(n * (int64_t)(G.Nc + G.Nf) * 4);
    L.g_raw_s = ws.take(G.shared ? n * G.Nf * 4 : 0);
    L.range_params = ws.take(sz_params);
    L.fine_total = ws.take(G.shared && G.Nf > 0 ? param_floats(P[0].kind) : 0);
    L.film_pass = ws.take(any_film ? G.n_groups * film_fl : 0);
    L.film_row = ws.take(any_film ? film_fl : 0);
    L.acts = ws.take(sz_acts);
    L.raw = ws.take(sz_raw);
    L.grads = ws.take(sz_grads);
    L.partial = ws.take(sz_part);
    L.film_partial = ws.take(sz_fpart);
    L.total = ws.floats;
    return L;
}

// The forward's state in the mi_render_rays workspace (one field adds z_samples, raw_samples, pos).
using State = RenderWorkspace::Regions;

static State carve_state(void* workspace, const RenderCall& G) { return RenderWorkspace(G.n, G.Nc, G.Nf).carve(workspace); }

// Checks shared by the size queries and both entry points.  shared: one field for both passes.
static int check_common(const char* fn, int kind_c, int kind_f, int64_t n_groups, int64_t rpg, int nc, int nf,
                        int64_t rp_c, int64_t rp_f) {
    if (bad_kind(kind_c) || bad_kind(kind_f)) return MI_EINVAL;
    if (is_film(kind_c) && is_film(kind_f) && film_layers(kind_c) != film_layers(kind_f)) {
        set_error("%s: the two FiLM fields of one call share the FiLM table, so they need the same depth (%d and %d rows)", fn,
                  film_layers(kind_c), film_layers(kind_f));
        return MI_EINVAL;
    }
    if (n_groups < 0 || rpg < 0 || nc < 3 || nf < 0) {
        set_error("%s: bad sizes (need n_groups, rays_per_group >= 0, Nc >= 3, Nf >= 0)", fn);
        return MI_EINVAL;
    }
    if (rp_c <= 0 || rp_f <= 0) {
        set_error("%s: points per range must be positive (coarse %lld, fine %lld)", fn, (long long)rp_c, (long long)rp_f);
        return MI_EINVAL;
    }
    return MI_OK;
}

static int check_state(const char* fn, const RenderCall& G, int64_t workspace_bytes, const void* saved, int64_t saved_bytes) {
    const RenderWorkspace layout(G.n, G.Nc, G.Nf);
    const int64_t need = layout.base_bytes() + (G.shared ? layout.shared_extra_bytes() : 0);
    if (workspace_bytes < need) {
        set_error("%s: workspace of %lld bytes, need %lld (mi_render_workspace_bytes%s)", fn, (long long)workspace_bytes,
                  (long long)need, G.shared ? " + mi_render_shared_field_extra_bytes: one field for both passes" : "");
        return MI_EINVAL;
    }
    if (saved_bytes < 0 || (saved_bytes > 0 && !saved)) {
        set_error("%s: saved buffer of %lld bytes at %p", fn, (long long)saved_bytes, saved);
        return MI_EINVAL;
    }
    return MI_OK;
}

// One pass of the training forward (autograd._forward_pass): the kept ranges through the saving kernel, the rest
// through the plain one (finishing the image the kept ranges stopped inside first).  raw [n,S,4].
static int forward_pass(const PassSpec& P, const RenderCall& G, const float* packed, const float* film, const float* rays,
                        const float* z, float* raw, int64_t kept, float*& saved, hipStream_t hs) {
    const Ranges R = make_ranges(P.kind, G.n_groups, G.rays_per_group, P.S, P.range_points);
    const int64_t acts = region_total(field_kind(P.kind).acts);
    const int64_t film_fl = film_floats(P.kind);   // one group's rows of the FiLM table
    const int S = P.S;
    int64_t r_done = 0;
    int rc;
    for (int64_t k = 0; k < kept; ++k) {
        int64_t r0, r1, g0, ng;
        R.get(k, r0, r1);
        range_groups(R, r0, r1, g0, ng);
        if ((rc = eval_field_rays(P.kind, packed, R.film ? film + g0 * film_fl : nullptr, rays + r0 * 6, z + r0 * S, ng,
                                  (r1 - r0) / ng, S, raw + r0 * S * 4, hs, saved))) return rc;
        saved += acts * (r1 - r0) * S;
        r_done = r1;
    }
    if (r_done < R.n && R.film && r_done % R.rpg) {
        const int64_t r_next = (r_done / R.rpg + 1) * R.rpg;
        if ((rc = eval_field_rays(P.kind, packed, film + (r_done / R.rpg) * film_fl, rays + r_done * 6, z + r_done * S, 1,
                                  r_next - r_done, S, raw + r_done * S * 4, hs))) return rc;
        r_done = r_next;
    }
    if (r_done < R.n) {
        const int64_t ng = R.film ? (R.n - r_done) / R.rpg : 1;
        if ((rc = eval_field_rays(P.kind, packed, R.film ? film + (r_done / R.rpg) * film_fl : nullptr, rays + r_done * 6,
                                  z + r_done * S, ng, (R.n - r_done) / ng, S, raw + r_done * S * 4, hs))) return rc;
    }
    return MI_OK;
}

// Parameter-gradient pointers of a kind laid out in a scratch region (param_floats order).
void scratch_params(int kind, float* base, float* out[2 * kMaxLayers]) {
    for (int i = 0; i < 2 * field_kind(kind).n_layers; ++i) {
        out[i] = base;
        base += align64(param_numel(kind, i));
    }
}

// dst[i] += src[i] over a kind's parameter gradients (_foreach_add_): entered into acc, whose flush the caller owns, so
// that a FiLM row or table that belongs to the same sum goes out in the same launch
static int add_param_grads(Accumulator& acc, int kind, float* const* dst, float* const* src) {
    for (int i = 0; i < 2 * field_kind(kind).n_layers; ++i)
        if (int rc = acc.add(dst[i], src[i], param_numel(kind, i))) return rc;
    return MI_OK;
}

// ... and as a launch of its own
int add_param_grads(int kind, float* const* dst, float* const* src, hipStream_t stream) {
    Accumulator acc(stream);
    if (int rc = add_param_grads(acc, kind, dst, src)) return rc;
    return acc.flush();
}

struct PassIO {
    const float* packed;
    const float* packed_bwd;
    const float* const* params;
    const float* z;
    const float* raw;
    const float* g_raw;
    const float* saved;
    int64_t kept;
};

// One pass of the backward (autograd._field_backward): range by range, gradients to dst (n_params device pointers) and,
// FiLM kinds, the pass's table gradient to film_dst [n_groups,9,512].
static int backward_pass(const PassSpec& P, const RenderCall& G, const PassIO& io, const float* film, const float* rays,
                         float* const* dst, float* film_dst, float* bws, const BwdLayout& L, hipStream_t hs) {
    const Ranges R = make_ranges(P.kind, G.n_groups, G.rays_per_group, P.S, P.range_points);
    const FieldKind& K = field_kind(P.kind);
    const int64_t film_fl = film_floats(P.kind);   // one group's rows of the FiLM table
    const int64_t acts_f = region_total(K.acts);
    const int S = P.S;
    float* range_out[2 * kMaxLayers];
    scratch_params(P.kind, bws + L.range_params, range_out);
    const float* saved = io.saved;
    int rc;
    for (int64_t k = 0, count = R.count(); k < count; ++k) {
        int64_t r0, r1, g0, ng;
        R.get(k, r0, r1);
        range_groups(R, r0, r1, g0, ng);
        const int64_t pts = (r1 - r0) * S;
        const bool add_to_row = R.film && (r1 - r0) < R.rpg && r0 % R.rpg != 0;   // a later part of one image
        const float* f_c = R.film ? film + g0 * film_fl : nullptr;
        float* g_c = !R.film ? nullptr : add_to_row ? bws + L.film_row : film_dst + g0 * film_fl;
        const float* acts;
        const float* raw_k;
        if (k < io.kept) {
            acts = saved;
            raw_k = io.raw + r0 * S * 4;
            saved += acts_f * pts;
        } else {
            if ((rc = eval_field_rays(P.kind, io.packed, f_c, rays + r0 * 6, io.z + r0 * S, ng, (r1 - r0) / ng, S, bws + L.raw, hs,
                                      bws + L.acts))) return rc;
            acts = bws + L.acts;
            raw_k = bws + L.raw;
        }
        float* const* out = k == 0 ? dst : range_out;
        if ((rc = launch_field_backward(P.kind, io.packed_bwd, acts, bws + L.grads, raw_k, io.g_raw + r0 * S * 4, ng,
                                        pts / ng, f_c, R.film ? bws + L.film_partial : nullptr, g_c, bws + L.partial, out,
                                        R.film ? io.params : nullptr, hs))) return rc;
        if (k > 0) {                                   // _foreach_add_(total, out); a later part adds to its image's row
            Accumulator acc(hs);
            if ((rc = add_param_grads(acc, P.kind, dst, range_out))) return rc;
            if (add_to_row) acc.add(film_dst + g0 * film_fl, bws + L.film_row, film_fl);
            if ((rc = acc.flush())) return rc;
        }
    }
    return MI_OK;
}

}  // namespace mi

using namespace mi;

extern "C" {

int64_t mi_render_train_saved_bytes(int kind_coarse, int kind_fine, int shared, int64_t n, int n_coarse, int n_fine) {
    if (bad_kind(kind_coarse) || bad_kind(kind_fine)) return MI_EINVAL;
    if (n < 0 || n_coarse < 1 || n_fine < 0) { set_error("mi_render_train_saved_bytes: bad sizes"); return MI_EINVAL; }
    const int64_t coarse = region_total(field_kind(kind_coarse).acts) * n * n_coarse;
    const int64_t second = shared ? region_total(field_kind(kind_coarse).acts) * n * n_fine
                                  : region_total(field_kind(kind_fine).acts) * n * ((int64_t)n_coarse + n_fine);
    return 4 * (coarse + second);
}

int64_t mi_render_backward_workspace_bytes(int kind_coarse, int kind_fine, int shared, int64_t n_groups,
                                           int64_t rays_per_group, int n_coarse, int n_fine, int64_t range_points_coarse,
                                           int64_t range_points_fine) {
    if (int rc = check_common("mi_render_backward_workspace_bytes", kind_coarse, kind_fine, n_groups, rays_per_group,
                              n_coarse, n_fine, range_points_coarse, range_points_fine)) return rc;
    const RenderCall G(n_groups, rays_per_group, n_coarse, n_fine, shared != 0);
    if (G.n == 0) return 0;
    PassSpec P[2];
    pass_specs(kind_coarse, shared ? kind_coarse : kind_fine, G, range_points_coarse, range_points_fine, P);
    return bwd_layout(P, G).total * (int64_t)sizeof(float);
}

int mi_render_rays_train(int kind_coarse, const float* packed_coarse, int kind_fine, const float* packed_fine,
                         const float* film, const float* rays, int64_t n_groups, int64_t rays_per_group, float near_,
                         float far_, int n_coarse, int n_fine, const float* z_lin, const float* u_lin, const float* t_rand,
                         uint64_t seed, uint64_t ray0, float* rgb_c, float* depth_c, float* acc_c, float* rgb_f,
                         float* depth_f, float* acc_f, void* workspace, int64_t workspace_bytes,
                         int64_t range_points_coarse, int64_t range_points_fine, void* saved, int64_t saved_bytes,
                         void* stream) {
    const char* fn = "mi_render_rays_train";
    if (int rc = check_common(fn, kind_coarse, kind_fine, n_groups, rays_per_group, n_coarse, n_fine, range_points_coarse,
                              range_points_fine)) return rc;
    const bool shared = one_field(kind_coarse, packed_coarse, kind_fine, packed_fine);
    const RenderCall G(n_groups, rays_per_group, n_coarse, n_fine, shared);
    if (G.n == 0) return MI_OK;
    if (!workspace || !rays || !packed_coarse || !packed_fine || !rgb_c || !depth_c || !acc_c || !rgb_f || !depth_f || !acc_f) {
        set_error("%s: null pointer argument", fn);
        return MI_EINVAL;
    }
    if ((is_film(kind_coarse) || is_film(kind_fine)) && !film) { set_error("%s: FiLM kind needs a film table", fn); return MI_EINVAL; }
    if (int rc = check_state(fn, G, workspace_bytes, saved, saved_bytes)) return rc;
    PassSpec P[2];
    pass_specs(kind_coarse, kind_fine, G, range_points_coarse, range_points_fine, P);
    int64_t kept[2];
    plan_kept(P, G, saved_bytes, kept);
    float* sv = (float*)saved;
    hipStream_t hs = (hipStream_t)stream;
    // the sequence of mi_render_rays, with field steps that keep their layer inputs; check_state demands the shared-field
    // regions of one field, so its fine pass is the Nf new depths (or, with Nf = 0, the coarse pass)
    const auto coarse_field = [&](const float* z, int, float* raw) { return forward_pass(P[0], G, packed_coarse, film, rays, z, raw, kept[0], sv, hs); };
    const auto fine_field = [&](const float* z, int, float* raw) { return forward_pass(P[1], G, packed_fine, film, rays, z, raw, kept[1], sv, hs); };
    const RenderIO io{rays, near_, far_, z_lin, u_lin, t_rand, seed, ray0, rgb_c, depth_c, acc_c, rgb_f, depth_f, acc_f};
    return run_render_passes(fn, G, fine_plan(shared, n_fine, true), io, carve_state(workspace, G), COARSE_RAW, coarse_field, fine_field, hs);
}

int mi_render_rays_backward(int kind_coarse, const float* packed_coarse, const float* packed_bwd_coarse,
                            const float* const* params_coarse, int kind_fine, const float* packed_fine,
                            const float* packed_bwd_fine, const float* const* params_fine, const float* film,
                            const float* rays, int64_t n_groups, int64_t rays_per_group, int n_coarse, int n_fine,
                            int64_t range_points_coarse, int64_t range_points_fine, const void* workspace,
                            int64_t workspace_bytes, const void* saved, int64_t saved_bytes, const float* g_rgb_c,
                            const float* g_depth_c, const float* g_acc_c, const float* g_rgb_f, const float* g_depth_f,
                            const float* g_acc_f, float* const* grad_params_coarse, float* const* grad_params_fine,
                            float* grad_film, void* bwd_workspace, int64_t bwd_workspace_bytes, int* fields_written,
                            void* stream) {
    const char* fn = "mi_render_rays_backward";
    if (fields_written) *fields_written = 0;
    if (int rc = check_common(fn, kind_coarse, kind_fine, n_groups, rays_per_group, n_coarse, n_fine, range_points_coarse,
                              range_points_fine)) return rc;
    const bool shared = one_field(kind_coarse, packed_coarse, kind_fine, packed_fine);
    const RenderCall G(n_groups, rays_per_group, n_coarse, n_fine, shared);
    if (G.n == 0) return MI_OK;
    const bool want_c = g_rgb_c || g_depth_c || g_acc_c;
    const bool want_f = g_rgb_f || g_depth_f || g_acc_f;
    // which fields receive gradients (_RenderRaysFn.backward's want_c / want_f): one field gets both passes' worth
    const bool run_c = shared ? (want_c || want_f) : want_c;
    const bool run_f = shared ? (want_f && n_fine > 0) : want_f;
    if (!workspace || !rays || !packed_coarse || !packed_fine) { set_error("%s: null pointer argument", fn); return MI_EINVAL; }
    const int kinds[2] = {kind_coarse, kind_fine};
    const float* const* params[2] = {params_coarse, params_fine};
    const float* packed_bwd[2] = {packed_bwd_coarse, packed_bwd_fine};
    float* const* grads[2] = {grad_params_coarse, shared ? nullptr : grad_params_fine};
    const bool runs[2] = {run_c, shared ? run_f : want_f};
    bool film_written = false;
    for (int f = 0; f < (shared ? 1 : 2); ++f) {
        const int np = 2 * field_kind(kinds[f]).n_layers;
        const char* which = f ? "fine" : "coarse";
        if (is_film(kinds[f])) {
            if (!film) { set_error("%s: FiLM kind needs a film table", fn); return MI_EINVAL; }
            if (!params[f]) { set_error("%s: FiLM kinds need the %s field's parameter array", fn, which); return MI_EINVAL; }
            for (int i = 0; i < np; ++i)
                if (!params[f][i]) { set_error("%s: %s parameter pointer %d is null", fn, which, i); return MI_EINVAL; }
        }
        if (!runs[f]) continue;
        if (int rc = check_field_grads(fn, which, kinds[f], packed_bwd[f], grads[f])) return rc;
        if (is_film(kinds[f]) && !grad_film) { set_error("%s: FiLM kind needs grad_film", fn); return MI_EINVAL; }
    }
    if (int rc = check_state(fn, G, workspace_bytes, saved, saved_bytes)) return rc;
    PassSpec P[2];
    pass_specs(kind_coarse, kind_fine, G, range_points_coarse, range_points_fine, P);
    const BwdLayout L = bwd_layout(P, G);
    if (bwd_workspace_bytes < L.total * (int64_t)sizeof(float) || !bwd_workspace) {
        set_error("%s: backward workspace of %lld bytes, mi_render_backward_workspace_bytes says %lld", fn,
                  (long long)bwd_workspace_bytes, (long long)(L.total * (int64_t)sizeof(float)));
        return MI_EINVAL;
    }
    if (!run_c && !run_f) return MI_OK;
    int64_t kept[2];
    const float* saved_f = (const float*)saved;
    const float* saved_pass[2] = {saved_f, saved_f + plan_kept(P, G, saved_bytes, kept)};
    const State st = carve_state(const_cast<void*>(workspace), G);
    float* bws = (float*)bwd_workspace;
    const int64_t n = G.n;
    const int S = n_coarse + n_fine;
    hipStream_t hs = (hipStream_t)stream;
    float* g_raw_c = bws + L.g_raw_c;
    float* g_raw_f = bws + L.g_raw_f;
    int rc;
    if (!shared) {
        if (want_c) {
            if ((rc = launch_composite_bwd(n, n_coarse, st.raw_c, st.z_c, rays, g_rgb_c, g_depth_c, g_acc_c, nullptr, g_raw_c,
                                           hs))) return rc;
            const PassIO io{packed_coarse, packed_bwd_coarse, params_coarse, st.z_c, st.raw_c, g_raw_c, saved_pass[0], kept[0]};
            if ((rc = backward_pass(P[0], G, io, film, rays, grad_params_coarse, grad_film, bws, L, hs))) return rc;
            film_written = is_film(kind_coarse);
        }
        if (want_f) {
            if ((rc = launch_composite_bwd(n, S, st.raw_f, st.z_f, rays, g_rgb_f, g_depth_f, g_acc_f, nullptr, g_raw_f, hs)))
                return rc;
            const PassIO io{packed_fine, packed_bwd_fine, params_fine, st.z_f, st.raw_f, g_raw_f, saved_pass[1], kept[1]};
            float* film_dst = film_written ? bws + L.film_pass : grad_film;
            if ((rc = backward_pass(P[1], G, io, film, rays, grad_params_fine, film_dst, bws, L, hs))) return rc;
            if (film_written && is_film(kind_fine)) {          // grad_film = coarse pass + fine pass
                Accumulator acc(hs);
                acc.add(grad_film, bws + L.film_pass, n_groups * film_floats(kind_coarse));
                if ((rc = acc.flush())) return rc;
            }
            film_written |= is_film(kind_fine);
        }
        if (fields_written) *fields_written = fields_written_word(false, want_c, want_f, film_written);
        return MI_OK;
    }
    // one field: the coarse points get what the coarse outputs and the fine outputs send them (mi_split_grad), the new
    // samples get the rest; each set goes through the field's backward once and the two totals are added
    const float* g_c = g_raw_c;
    if (want_c && (rc = launch_composite_bwd(n, n_coarse, st.raw_c, st.z_c, rays, g_rgb_c, g_depth_c, g_acc_c, nullptr, g_raw_c,
                                             hs))) return rc;
    if (want_f) {
        const bool fine_sorted = n_fine > 0;                   // Nf = 0: the fine pass is the coarse pass
        if ((rc = launch_composite_bwd(n, fine_sorted ? S : n_coarse, fine_sorted ? st.raw_f : st.raw_c,
                                   fine_sorted ? st.z_f : st.z_c, rays, g_rgb_f, g_depth_f, g_acc_f, nullptr, g_raw_f,
                                       hs))) return rc;
        if (fine_sorted) {
            if ((rc = launch_split_grad(n, n_coarse, n_fine, g_raw_f, st.pos, g_raw_c, want_c ? 1 : 0, bws + L.g_raw_s, hs)))
                return rc;
        } else if (want_c) {                                   // g_raw = coarse g_raw + fine g_raw
            Accumulator acc(hs);
            acc.add(g_raw_c, g_raw_f, n * n_coarse * 4);
            if ((rc = acc.flush())) return rc;
        } else {
            g_c = g_raw_f;
        }
    }
    const PassIO io_c{packed_coarse, packed_bwd_coarse, params_coarse, st.z_c, st.raw_c, g_c, saved_pass[0], kept[0]};
    if ((rc = backward_pass(P[0], G, io_c, film, rays, grad_params_coarse, grad_film, bws, L, hs))) return rc;
    if (run_f) {
        float* fine_total[2 * kMaxLayers];
        scratch_params(kind_coarse, bws + L.fine_total, fine_total);
        const PassIO io_s{packed_coarse, packed_bwd_coarse, params_coarse, st.z_s, st.raw_s, bws + L.g_raw_s, saved_pass[1],
                          kept[1]};
        const bool film_kind = is_film(kind_coarse);
        if ((rc = backward_pass(P[1], G, io_s, film, rays, fine_total, film_kind ? bws + L.film_pass : nullptr, bws, L,
                                hs))) return rc;
        Accumulator acc(hs);                                   // _foreach_add_(grads_c, grads_f); grad_film += fine pass's
        if ((rc = add_param_grads(acc, kind_coarse, grad_params_coarse, fine_total))) return rc;
        if (film_kind) acc.add(grad_film, bws + L.film_pass, n_groups * film_floats(kind_coarse));
        if ((rc = acc.flush())) return rc;
    }
    if (fields_written) *fields_written = fields_written_word(true, true, false, is_film(kind_coarse));
    return MI_OK;
}

}  // extern "C"
