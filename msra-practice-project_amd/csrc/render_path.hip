// render_path.hip - the plain render path of the C ABI (include/mi_render.h): mi_render_rays and its size queries, the two
// field steps that only it has - the windowed sigma-only coarse pass and the fine pass's deferred colour branch
// (mi_field_eval_rays_deferred exports the latter) - and the MLP-event hook.  Also the out-of-line helpers of render_path.h
// that belong to no single path.  Host code only: this unit holds no kernel.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "render_path.h"

namespace mi {

static thread_local hipEvent_t g_mlp_ev[4] = {nullptr, nullptr, nullptr, nullptr};

int copy_render_outputs(const char* fn, int64_t n, float* rgb_dst, float* depth_dst, float* acc_dst, const float* rgb_src,
                        const float* depth_src, const float* acc_src, hipStream_t stream) {
    const struct { float* dst; const float* src; int64_t floats; } copies[3] = {
        {rgb_dst, rgb_src, n * 3}, {depth_dst, depth_src, n}, {acc_dst, acc_src, n}};
    for (const auto& c : copies)
        if (c.dst && hipMemcpyAsync(c.dst, c.src, c.floats * sizeof(float), hipMemcpyDeviceToDevice, stream) != hipSuccess) {
            set_error("%s: output alias copy failed", fn);
            return MI_EHIP;
        }
    return MI_OK;
}

int check_field_grads(const char* fn, const char* which, int kind, const float* packed_bwd, float* const* grads) {
    if (!packed_bwd) { set_error("%s: the %s field has no transposed stream", fn, which); return MI_EINVAL; }
    if (!grads) { set_error("%s: the %s field gets a cotangent but has no gradient array", fn, which); return MI_EINVAL; }
    for (int i = 0; i < 2 * field_kind(kind).n_layers; ++i)
        if (!grads[i]) { set_error("%s: %s gradient pointer %d is null", fn, which, i); return MI_EINVAL; }
    return MI_OK;
}

// Samples per window of the sigma-only coarse pass of mi_render_rays (a power of two that divides 128, the point tile).
#ifndef MI_COARSE_WINDOW_LOG2
#define MI_COARSE_WINDOW_LOG2 3
#endif
constexpr int kCoarseWindowLog2 = MI_COARSE_WINDOW_LOG2;
constexpr int kCoarseWindow = 1 << kCoarseWindowLog2;
static_assert(kCoarseWindow >= 1 && 128 % kCoarseWindow == 0, "a tile is 128 / kCoarseWindow rays x one window");

// The sigma-only coarse pass, front to back in windows of kCoarseWindow samples: window r evaluates the field at its
// samples of the rays that are still live, then the resumable weights composite (render_stages.hip) writes the window's
// weights and drops every ray whose transmittance has reached zero - all its later weights are exactly 0 whatever the
// field says there, so the field is not asked.  Same weights / depth_c / acc_c bits as one whole pass.  A caller that
// asks for neither depth_c nor acc_c leaves sample_fine as the weights' only reader, and a ray is dropped as soon as no
// later weight can change w + kPdfEps there (kStopBelowPdfEps, launchers.h): same z_fine bits, far fewer points.
// Everything is launched with worst-case grids from host values only (no read-back: graph-capturable); `scratch` is the
// part of raw_c's region behind the compact sigma buffer: two live lists [n] and one count per window.
static int coarse_sigma_windows(int kind, const float* packed, const float* rays, const float* z_c, int64_t n, int n_coarse,
                                float* sigma, int* scratch, float* depth_c, float* acc_c, float* w_c, hipStream_t hs) {
    const int rounds = (n_coarse + kCoarseWindow - 1) / kCoarseWindow;
    int* list[2] = {scratch, scratch + n};
    int* counts = scratch + 2 * n;
    const double stop = depth_c || acc_c ? kStopZeroWeight : kStopBelowPdfEps;
    if (int rc = launch_clear_floats(rounds, (float*)counts, hs)) return rc;     // render_stages.hip: why not a memset node
    MlpArgs args = {};
    args.packed = packed; args.a = rays; args.z = z_c; args.out = sigma;
    args.n_samples = n_coarse; args.mode = 1; args.n_rays = n; args.win_log2 = kCoarseWindowLog2;
    for (int r = 0; r < rounds; ++r) {
        const int k0 = r * kCoarseWindow, k1 = k0 + kCoarseWindow < n_coarse ? k0 + kCoarseWindow : n_coarse;
        const bool last = r == rounds - 1;
        args.live_rays = r ? list[r & 1] : nullptr;          // window 0: every ray
        args.live_count = r ? counts + r : nullptr;
        args.win_k0 = k0;
        int rc;
        if ((rc = launch_mlp_window(kind, args, hs))) return rc;
        if ((rc = launch_composite_weights_window(n, n_coarse, sigma, z_c, rays, depth_c, acc_c, w_c, args.live_rays,
                                                  args.live_count, last ? nullptr : list[(r + 1) & 1],
                                                  last ? nullptr : counts + r + 1, k0, k1, stop, hs))) return rc;
    }
    return MI_OK;
}

// Points per chunk of the fine pass's deferred colour branch (the row buffer holds that many 1 KiB rows).
#ifndef MI_COLOUR_CHUNK_ROWS_LOG2
#define MI_COLOUR_CHUNK_ROWS_LOG2 22
#endif
constexpr int64_t kColourChunkRows = (int64_t)1 << MI_COLOUR_CHUNK_ROWS_LOG2;
static int64_t g_colour_chunk_rows = 0;               // mi_render_set_colour_chunk_rows: 0 = kColourChunkRows
static int64_t colour_chunk_rows() { return g_colour_chunk_rows > 0 ? g_colour_chunk_rows : kColourChunkRows; }

// kinds with the two kernels, point indices that fit the live list's ints
static bool can_defer_colour(int kind, int64_t n, int S) { return has_deferred_colour_kernels(kind) && n > 0 && S > 0 && n * S <= 0x7fffffffLL; }

// The field over n rays of S samples with its colour branch deferred to the points with sigma > 0, in chunks of whole rays:
// per chunk a trunk-and-spill launch ({0, 0, 0, sigma} for every point, H8 rows and indices of the live ones into `extra`)
// and a colour launch over that list.  A point with sigma == 0 keeps r = g = b = 0: its weight is exactly 0, so 0 * rgb
// is the +0 that any finite colour gives.  Every chunk has its own count, cleared by one kernel launch; all launches on `hs`
// with grids from host values (no read-back: graph-capturable).  `extra`: DeferredColourBuf(n, S, colour_chunk_rows()).
static int eval_rays_deferred_colour(int kind, const float* packed, const float* rays, const float* z, int64_t n, int S,
                                     float* raw, void* extra, hipStream_t hs) {
    const DeferredColourBuf buf(n, S, colour_chunk_rows());
    const DeferredColourBuf::Regions r = buf.carve(extra);
    if (int rc = launch_clear_floats(buf.n_chunks, (float*)r.counts, hs)) return rc;
    MlpArgs args = {};
    args.packed = packed; args.n_samples = S; args.mode = 1;
    for (int64_t i = 0; i < buf.n_chunks; ++i) {
        const int64_t r0 = i * buf.chunk_rays, nr = n - r0 < buf.chunk_rays ? n - r0 : buf.chunk_rays;
        args.a = rays + r0 * 6; args.z = z + r0 * S; args.out = raw + r0 * S * 4;
        args.rays_per_group = nr; args.points_per_group = nr * S; args.tiles_per_group = (nr * S + 127) / 128;
        args.save_points = nr * S;
        const DeferArgs d = {r.rows, r.idx, r.counts + i};
        int rc;
        if ((rc = launch_mlp_trunk_spill(kind, args, d, hs))) return rc;
        if ((rc = launch_mlp_colour(kind, args, d, hs))) return rc;
    }
    return MI_OK;
}

// bad_kind's refusal, with the call's name in front of it
static bool bad_kind_in(const char* fn, int kind) {
    if (!bad_kind(kind)) return false;
    char why[400];
    snprintf(why, sizeof(why), "%s", mi_last_error());
    set_error("%s: %s", fn, why);
    return true;
}

}  // namespace mi

using namespace mi;

extern "C" {

int64_t mi_render_deferred_colour_extra_bytes(int64_t n, int n_coarse, int n_fine) {
    if (n <= 0 || n_coarse < 1 || n_fine <= 0) return 0;
    return DeferredColourBuf(n, (int64_t)n_coarse + n_fine, colour_chunk_rows()).bytes();
}

void mi_render_set_colour_chunk_rows(int64_t rows) { g_colour_chunk_rows = rows > 0 ? rows : 0; }

int mi_field_eval_rays_deferred(int kind, const float* packed, const float* film, const float* rays, const float* z,
                                int64_t n_groups, int64_t rays_per_group, int n_samples, float* raw, void* extra,
                                int64_t extra_bytes, void* stream) {
    (void)film;
    if (bad_kind(kind)) return MI_EINVAL;
    if (n_samples <= 0 || n_groups < 0 || rays_per_group < 0) { set_error("mi_field_eval_rays_deferred: bad sizes"); return MI_EINVAL; }
    const int64_t n = n_groups * rays_per_group;
    if (n == 0) return MI_OK;
    if (!packed || !rays || !z || !raw || !extra) { set_error("mi_field_eval_rays_deferred: null pointer argument"); return MI_EINVAL; }
    if (!can_defer_colour(kind, n, n_samples)) {
        set_error("mi_field_eval_rays_deferred: kind %d has no deferred colour branch, or n * n_samples exceeds 2^31 - 1", kind);
        return MI_EINVAL;
    }
    const int64_t need = DeferredColourBuf(n, n_samples, colour_chunk_rows()).bytes();
    if (extra_bytes < need) {
        set_error("mi_field_eval_rays_deferred: buffer of %lld bytes, needs %lld", (long long)extra_bytes, (long long)need);
        return MI_EINVAL;
    }
    return eval_rays_deferred_colour(kind, packed, rays, z, n, n_samples, raw, extra, (hipStream_t)stream);
}

int64_t mi_render_workspace_bytes(int64_t n, int n_coarse, int n_fine) {
    return RenderWorkspace(n, n_coarse, n_fine).base_bytes();
}

int64_t mi_render_shared_field_extra_bytes(int64_t n, int n_coarse, int n_fine) {
    return RenderWorkspace(n, n_coarse, n_fine).shared_extra_bytes();
}

int mi_render_rays(int kind_coarse, const float* packed_coarse, int kind_fine, const float* packed_fine,
                   const float* film, const float* rays, int64_t n_groups, int64_t rays_per_group, float near_,
                   float far_, int n_coarse, int n_fine, const float* z_lin, const float* u_lin, const float* t_rand,
                   uint64_t seed, uint64_t ray0, float* rgb_c, float* depth_c, float* acc_c, float* rgb_f,
                   float* depth_f, float* acc_f, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* fn = "mi_render_rays";
    if (n_groups < 0 || rays_per_group < 0 || n_coarse < 1 || n_fine < 0) { set_error("mi_render_rays: bad sizes"); return MI_EINVAL; }
    if (n_groups * rays_per_group == 0) return MI_OK;          // no rays: nothing to launch, no buffer is touched
    // the coarse outputs are optional: rgb_c NULL = the coarse colours are not wanted, and then depth_c / acc_c each may be
    // NULL too; with rgb_c, all three
    if (!workspace || !rays || !packed_coarse || !packed_fine || (rgb_c && (!depth_c || !acc_c)) || !rgb_f || !depth_f || !acc_f) {
        set_error("mi_render_rays: null pointer argument");
        return MI_EINVAL;
    }
    if (bad_kind_in(fn, kind_coarse) || bad_kind_in(fn, kind_fine)) return MI_EINVAL;
    if ((is_film(kind_coarse) || is_film(kind_fine)) && !film) { set_error("mi_render_rays: FiLM kind needs a film table"); return MI_EINVAL; }
    const RenderCall C(n_groups, rays_per_group, n_coarse, n_fine, one_field(kind_coarse, packed_coarse, kind_fine, packed_fine));
    const int64_t n = C.n;
    const RenderWorkspace layout(n, n_coarse, n_fine);
    const int64_t base_bytes = layout.base_bytes();
    // One field in a workspace that lacks the shared-field regions gets the whole fine pass (same results).
    const FinePlan plan = fine_plan(C.shared, n_fine, workspace_bytes >= base_bytes + layout.shared_extra_bytes());
    // sample_pdf is called with mids (Nc-1 bins) and weights[1:-1] (Nc-2)
    if (plan != FINE_IS_COARSE && n_coarse < 3) {
        set_error("mi_render_rays: need Nc >= 3 to sample a fine pass (Nc = %d serves one field with Nf = 0 only)", n_coarse);
        return MI_EINVAL;
    }
    if (workspace_bytes < base_bytes) {
        set_error("mi_render_rays: workspace of %lld bytes, mi_render_workspace_bytes says %lld", (long long)workspace_bytes,
                  (long long)base_bytes);
        return MI_EINVAL;
    }
    const RenderWorkspace::Regions ws = layout.carve(workspace);
    hipStream_t hs = (hipStream_t)stream;
    // Without the coarse colours and with a coarse field of its own, the coarse pass only feeds sample_fine its weights,
    // which depend on sigma alone: the sigma-only forward writes sigma [n,Nc] compactly at the start of raw_c's region.
    // A shared field's coarse raw values are merged into the fine pass (or are its outputs with Nf = 0): whole forward.
    // The other three quarters of the region hold the windowed pass's live lists and counts: 2 n + ceil(Nc / window) ints
    // <= 3 n Nc floats whenever Nc >= 2.
    const bool sigma_only = !rgb_c && !C.shared && has_sigma_only_kernel(kind_coarse);
    // more than one window, and ray indices that fit the live lists' ints: the windowed pass (weights included)
    const bool windowed = sigma_only && n_coarse > kCoarseWindow && n <= 0x7fffffffLL;
    const auto coarse_field = [&](const float* z, int samples, float* raw) -> int {
        if (g_mlp_ev[0]) (void)hipEventRecord(g_mlp_ev[0], hs);
        const int rc = windowed ? coarse_sigma_windows(kind_coarse, packed_coarse, rays, z, n, samples, raw, (int*)(raw + n * samples),
                                                       depth_c, acc_c, ws.w_c, hs)
                                : eval_field(kind_coarse, packed_coarse, film, rays, z, n_groups, rays_per_group * samples,
                                             rays_per_group, samples, 1, raw, hs, nullptr, sigma_only);
        if (rc) return rc;
        if (g_mlp_ev[1]) (void)hipEventRecord(g_mlp_ev[1], hs);
        return MI_OK;
    };
    // A fine field of its own, in a workspace that also holds mi_render_deferred_colour_extra_bytes (behind base_bytes, where
    // the shared path's regions would lie): the colour branch runs on the points with sigma > 0 only.  A caller that did not
    // provide the extra gets the whole forward (same results).
    const int64_t defer_bytes = mi_render_deferred_colour_extra_bytes(n, n_coarse, n_fine);
    const bool deferred = !C.shared && defer_bytes > 0 && can_defer_colour(kind_fine, n, n_coarse + n_fine) &&
                          workspace_bytes >= base_bytes + defer_bytes;
    const auto fine_field = [&](const float* z, int samples, float* raw) -> int {
        if (g_mlp_ev[2]) (void)hipEventRecord(g_mlp_ev[2], hs);
        const int rc = deferred ? eval_rays_deferred_colour(kind_fine, packed_fine, rays, z, n, samples, raw, (char*)workspace + base_bytes, hs)
                                : eval_field_rays(kind_fine, packed_fine, film, rays, z, n_groups, rays_per_group, samples, raw, hs);
        if (rc) return rc;
        if (g_mlp_ev[3]) (void)hipEventRecord(g_mlp_ev[3], hs);
        return MI_OK;
    };
    const RenderIO io{rays, near_, far_, z_lin, u_lin, t_rand, seed, ray0, rgb_c, depth_c, acc_c, rgb_f, depth_f, acc_f};
    return run_render_passes(fn, C, plan, io, ws, windowed ? COARSE_WEIGHTS : sigma_only ? COARSE_SIGMA : COARSE_RAW, coarse_field,
                             fine_field, hs);
}

void mi_render_set_mlp_events(void* start_coarse, void* stop_coarse, void* start_fine, void* stop_fine) {
    g_mlp_ev[0] = (hipEvent_t)start_coarse; g_mlp_ev[1] = (hipEvent_t)stop_coarse;
    g_mlp_ev[2] = (hipEvent_t)start_fine; g_mlp_ev[3] = (hipEvent_t)stop_fine;
}
}  // extern "C"
