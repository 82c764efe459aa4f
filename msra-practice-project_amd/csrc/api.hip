// api.hip - the one-stage calls of libmirender.so's extern "C" surface (include/mi_render.h): error state, the field-kind
// registry, pack, the field and stage wrappers, metrics, loss, ray bank, Adam, events.  Argument validation lives here; kernels
// assume validated shapes.  The render paths are render_path.hip, train_path.hip and occupancy_path.hip.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#include "render_path.h"

namespace mi {

static thread_local char g_err[512] = "";
#ifdef MI_PROFILE_STAMPS
static unsigned long long* g_stamps = nullptr;
extern unsigned long long* g_bwd_stamps;          // field_bwd_chain.hip
#endif

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int check_launch(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return MI_EHIP;
    }
    return MI_OK;
}

const FieldKind& field_kind(int kind) {
    if (is_fixed_kind(kind)) return kFieldKinds[kind];
    struct DepthKinds {
        FieldKind k[kFilmDepthMax - kFilmDepthMin + 1][2];
        DepthKinds() {
            for (int L = kFilmDepthMin; L <= kFilmDepthMax; ++L)
                for (int d = 0; d < 2; ++d) k[L - kFilmDepthMin][d] = make_film_kind(L, d != 0);
        }
    };
    static const DepthKinds depth;                       // built once, on first use
    return depth.k[film_depth(kind) - kFilmDepthMin][kind & 1];
}

// one launch of the fused forward, arguments already checked (the render paths call it from their field steps)
int eval_field(int kind, const float* packed, const float* film, const float* a, const float* z, int64_t n_groups, int64_t ppg,
               int64_t rpg, int S, int mode, float* out, hipStream_t s, float* save, bool sigma_only) {
    MlpArgs args;
    args.packed = packed; args.film = is_film(kind) ? film : nullptr; args.a = a; args.z = z; args.out = out;
    args.points_per_group = ppg; args.rays_per_group = rpg; args.tiles_per_group = (ppg + 127) / 128;
    args.n_samples = S; args.mode = mode; args.save = save; args.save_points = n_groups * ppg;
    args.film_depth = film_depth(kind);
    args.live_rays = nullptr; args.live_count = nullptr; args.n_rays = 0; args.win_k0 = 0; args.win_log2 = 0;
#ifdef MI_PROFILE_STAMPS
    args.stamps = g_stamps;
#else
    args.stamps = nullptr;
#endif
    return launch_mlp(kind, args, n_groups, s, sigma_only);
}

// the checks of the one-stage field wrappers, then the launch
static int eval_common(int kind, const float* packed, const float* film, const float* a, const float* z,
                       int64_t n_groups, int64_t ppg, int64_t rpg, int S, int mode, float* out, hipStream_t s,
                       float* save = nullptr) {
    if (bad_kind(kind)) return MI_EINVAL;
    if (!packed || !a || !out || (mode == 1 && !z)) { set_error("null pointer argument"); return MI_EINVAL; }
    if (is_film(kind) && !film) { set_error("FiLM kind needs a film table"); return MI_EINVAL; }
    if (n_groups < 0 || ppg < 0) { set_error("negative size"); return MI_EINVAL; }
    if (n_groups == 0 || ppg == 0) return MI_OK;
    return eval_field(kind, packed, film, a, z, n_groups, ppg, rpg, S, mode, out, s, save);
}

}  // namespace mi

using namespace mi;

extern "C" {

int mi_abi_version(void) { return 4; }
const char* mi_last_error(void) { return g_err; }

int mi_field_num_params(int kind) { return bad_kind(kind) ? MI_EINVAL : 2 * field_kind(kind).n_layers; }
int64_t mi_field_packed_floats(int kind) { return bad_kind(kind) ? MI_EINVAL : packed_floats(field_kind(kind).fwd); }
int64_t mi_field_macs(int kind) { return bad_kind(kind) ? MI_EINVAL : field_kind(kind).macs(); }
int mi_field_film_layers(int kind) { return bad_kind(kind) ? MI_EINVAL : film_layers(kind); }
int mi_field_param_shape(int kind, int index, int64_t* rows, int64_t* cols) {
    if (bad_kind(kind)) return MI_EINVAL;
    const FieldKind& k = field_kind(kind);
    if (index < 0 || index >= 2 * k.n_layers || !rows || !cols) { set_error("mi_field_param_shape: bad arguments"); return MI_EINVAL; }
    *rows = k.dims[index / 2][0];
    *cols = (index & 1) ? 1 : k.dims[index / 2][1];
    return MI_OK;
}

// w_0 of the kind's sin layers: any finite w_0 > 0 for the FiLM kinds (FilmSiren's constructor argument, pi_GAN/modules.py:11,73);
// every other kind has no such parameter (Siren hard-codes 30, nerf/nerf.py:112; the ReLU kinds have no sin) and takes 30 only.
static int check_w0(int kind, float w_0, const char* fn) {
    if (is_film(kind)) {
        if (!(w_0 > 0.f) || !(w_0 < 1e30f)) { set_error("%s: w_0 = %g (FiLM kinds need a finite w_0 > 0)", fn, (double)w_0); return MI_EINVAL; }
    } else if (w_0 != 30.f) {
        set_error("%s: w_0 = %g, but only the FiLM kinds have a w_0 (pass 30 for kind %d)", fn, (double)w_0, kind);
        return MI_EINVAL;
    }
    return MI_OK;
}

int mi_field_pack(int kind, const float* const* params, int n_params, float w_0, float* packed, void* stream) {
    if (bad_kind(kind)) return MI_EINVAL;
    if (!params || !packed) { set_error("null pointer argument"); return MI_EINVAL; }
    if (n_params != 2 * field_kind(kind).n_layers) {
        set_error("kind %d expects %d parameter tensors, got %d", kind, 2 * field_kind(kind).n_layers, n_params);
        return MI_EINVAL;
    }
    for (int i = 0; i < n_params; ++i)
        if (!params[i]) { set_error("parameter %d is null", i); return MI_EINVAL; }
    if (int rc = check_w0(kind, w_0, "mi_field_pack")) return rc;
    return launch_pack(kind, STREAM_FWD, params, n_params, w_0, packed, (hipStream_t)stream);
}

int mi_field_eval_points(int kind, const float* packed, const float* film, const float* x, int64_t n_groups,
                         int64_t points_per_group, float* out, void* stream) {
    return eval_common(kind, packed, film, x, nullptr, n_groups, points_per_group, 0, 1, 0, out, (hipStream_t)stream);
}

int mi_field_eval_rays(int kind, const float* packed, const float* film, const float* rays, const float* z,
                       int64_t n_groups, int64_t rays_per_group, int n_samples, float* raw, void* stream) {
    if (n_samples <= 0) { set_error("n_samples must be positive"); return MI_EINVAL; }
    return eval_common(kind, packed, film, rays, z, n_groups, rays_per_group * n_samples, rays_per_group, n_samples, 1,
                       raw, (hipStream_t)stream);
}

int mi_field_has_deferred_colour(int kind) { return bad_kind(kind) ? MI_EINVAL : has_deferred_colour_kernels(kind) ? 1 : 0; }

int64_t mi_occupancy_words(const int* dims) {
    const int64_t cells = occupancy_cells("mi_occupancy_words", dims);
    return cells ? (cells + 31) / 32 : MI_EINVAL;
}

int64_t mi_occupancy_pack_workspace_bytes(const int* dims, int dilate) {
    const int64_t cells = occupancy_cells("mi_occupancy_pack_workspace_bytes", dims);
    if (!cells) return MI_EINVAL;
    if (dilate < 0) { set_error("mi_occupancy_pack_workspace_bytes: dilate = %d", dilate); return MI_EINVAL; }
    return occupancy_pack_workspace_bytes(cells, dilate);
}

int mi_occupancy_cell_points(const int* dims, const float* lo, const float* cell, int supersample, int64_t head, int64_t count,
                             float* points, void* stream) {
    const int64_t cells = occupancy_cells("mi_occupancy_cell_points", dims);
    if (!cells) return MI_EINVAL;
    if (!lo || !cell || supersample < 1 || supersample > 8 || head < 0 || count < 0 || head + count > cells || (count > 0 && !points)) {
        set_error("mi_occupancy_cell_points: bad arguments (need 1 <= supersample <= 8, 0 <= head, head + count <= cells)");
        return MI_EINVAL;
    }
    return launch_occupancy_cell_points(dims, lo, cell, supersample, head, count, points, (hipStream_t)stream);
}

int mi_occupancy_pack(const float* sigma, const int* dims, int supersample, float threshold, int dilate, uint32_t* bits,
                      void* workspace, int64_t workspace_bytes, void* stream) {
    const int64_t cells = occupancy_cells("mi_occupancy_pack", dims);
    if (!cells) return MI_EINVAL;
    if (!sigma || !bits || !workspace || supersample < 1 || supersample > 8 || dilate < 0) {
        set_error("mi_occupancy_pack: bad arguments (non-null sigma, bits, workspace; 1 <= supersample <= 8; dilate >= 0)");
        return MI_EINVAL;
    }
    const int64_t need = occupancy_pack_workspace_bytes(cells, dilate);
    if (workspace_bytes < need) {
        set_error("mi_occupancy_pack: workspace of %lld bytes, needs %lld", (long long)workspace_bytes, (long long)need);
        return MI_EINVAL;
    }
    return launch_occupancy_pack(sigma, dims, supersample, threshold, dilate, bits, workspace, (hipStream_t)stream);
}

int mi_occupancy_draw_points(const uint32_t* bits, const int* dims, const float* lo, const float* cell, uint64_t seed, uint32_t epoch,
                             int mode, int64_t row0, int64_t count, int64_t n_uniform, int* cell_ids, float* points, void* stream) {
    const char* fn = "mi_occupancy_draw_points";
    const int64_t cells = occupancy_cells(fn, dims);
    if (!cells) return MI_EINVAL;
    if ((mode != 0 && mode != 1) || row0 < 0 || count < 0 || n_uniform < 0 || row0 > (1LL << 31) - count) {
        set_error("%s: bad arguments (mode 0 or 1; row0, count, n_uniform >= 0; row0 + count <= 2^31)", fn);
        return MI_EINVAL;
    }
    if (mode == 0 && row0 + count > cells) {
        set_error("%s: a sweep of rows [%lld, %lld) over %lld cells", fn, (long long)row0, (long long)(row0 + count), (long long)cells);
        return MI_EINVAL;
    }
    const bool reads_bits = mode == 1 && n_uniform < row0 + count;
    if (!lo || !cell || !cell_ids || !points || (reads_bits && !bits)) { set_error("%s: null pointer argument", fn); return MI_EINVAL; }
    return launch_occupancy_draw_points(bits, dims, lo, cell, seed, epoch, mode, row0, count, n_uniform, cell_ids, points,
                                        (hipStream_t)stream);
}

int64_t mi_occupancy_density_workspace_bytes(const int* dims, int dilate) {
    const int64_t cells = occupancy_cells("mi_occupancy_density_workspace_bytes", dims);
    if (!cells) return MI_EINVAL;
    if (dilate < 0) { set_error("mi_occupancy_density_workspace_bytes: dilate = %d", dilate); return MI_EINVAL; }
    return occupancy_density_workspace_bytes(cells, dilate);
}

int mi_occupancy_density_update(const float* sigma, const int* cell_ids, int64_t count, const int* dims, float decay, float* density,
                                void* workspace, int64_t workspace_bytes, void* stream) {
    const char* fn = "mi_occupancy_density_update";
    const int64_t cells = occupancy_cells(fn, dims);
    if (!cells) return MI_EINVAL;
    if (!sigma || !cell_ids || !density || !workspace) { set_error("%s: null pointer argument", fn); return MI_EINVAL; }
    if (count < 0 || count > (1LL << 31)) { set_error("%s: count = %lld (0 .. 2^31)", fn, (long long)count); return MI_EINVAL; }
    if (!(decay >= 0.f && decay <= 1.f)) { set_error("%s: decay = %g (needs 0 <= decay <= 1)", fn, (double)decay); return MI_EINVAL; }
    const int64_t need = occupancy_density_workspace_bytes(cells, 0);
    if (workspace_bytes < need) {
        set_error("%s: workspace of %lld bytes, needs %lld", fn, (long long)workspace_bytes, (long long)need);
        return MI_EINVAL;
    }
    return launch_occupancy_density_update(sigma, cell_ids, count, dims, decay, density, workspace, (hipStream_t)stream);
}

int mi_occupancy_density_pack(const float* density, const int* dims, float threshold, int relative, int dilate, uint32_t* bits,
                              void* workspace, int64_t workspace_bytes, void* stream) {
    const char* fn = "mi_occupancy_density_pack";
    const int64_t cells = occupancy_cells(fn, dims);
    if (!cells) return MI_EINVAL;
    if (!density || !bits || !workspace) { set_error("%s: null pointer argument", fn); return MI_EINVAL; }
    if (dilate < 0) { set_error("%s: dilate = %d", fn, dilate); return MI_EINVAL; }
    const int64_t need = occupancy_density_workspace_bytes(cells, dilate);
    if (workspace_bytes < need) {
        set_error("%s: workspace of %lld bytes, needs %lld", fn, (long long)workspace_bytes, (long long)need);
        return MI_EINVAL;
    }
    return launch_occupancy_density_pack(density, dims, threshold, relative, dilate, bits, workspace, (hipStream_t)stream);
}

// n * n_samples points whose indices fit the list's ints
static int check_list_sizes(const char* fn, int64_t n, int n_samples) {
    if (n < 0 || n_samples < 1) { set_error("%s: bad sizes (n >= 0, n_samples >= 1)", fn); return MI_EINVAL; }
    if (n > 0x7fffffffLL / n_samples) {
        set_error("%s: n * n_samples = %lld * %d exceeds 2^31 - 1 (the list holds int point indices)", fn, (long long)n, n_samples);
        return MI_EINVAL;
    }
    return MI_OK;
}

// the two marks: the atomic one (any order) and the ordered one (ascending, what training needs)
static int mark_rays(const char* fn, bool ordered, const uint32_t* bits, const int* dims, const float* lo, const float* inv_cell,
                     const float* rays, const float* z, int64_t n, int n_samples, int* list, int* count, float* raw, void* stream) {
    OccupancyGridArgs grid;
    if (int rc = occupancy_grid_args(fn, bits, dims, lo, inv_cell, &grid)) return rc;
    if (!rays || !z || !list || !count) { set_error("%s: null pointer argument", fn); return MI_EINVAL; }
    if (int rc = check_list_sizes(fn, n, n_samples)) return rc;
    return (ordered ? launch_occupancy_mark_rays_ordered : launch_occupancy_mark_rays)(grid, rays, z, n, n_samples, list, count, raw,
                                                                                      (hipStream_t)stream);
}

int mi_occupancy_mark_rays(const uint32_t* bits, const int* dims, const float* lo, const float* inv_cell, const float* rays,
                           const float* z, int64_t n, int n_samples, int* list, int* count, float* raw, void* stream) {
    return mark_rays("mi_occupancy_mark_rays", false, bits, dims, lo, inv_cell, rays, z, n, n_samples, list, count, raw, stream);
}

int64_t mi_occupancy_ordered_list_ints(int64_t n, int n_samples) {
    if (check_list_sizes("mi_occupancy_ordered_list_ints", n, n_samples)) return MI_EINVAL;
    return occupancy_ordered_list_ints(n * n_samples);
}

int mi_occupancy_mark_rays_ordered(const uint32_t* bits, const int* dims, const float* lo, const float* inv_cell, const float* rays,
                                   const float* z, int64_t n, int n_samples, int* list, int* count, float* raw, void* stream) {
    return mark_rays("mi_occupancy_mark_rays_ordered", true, bits, dims, lo, inv_cell, rays, z, n, n_samples, list, count, raw, stream);
}

int mi_occupancy_clip_rays(const uint32_t* bits, const int* dims, const float* lo, const float* inv_cell, const float* rays, int64_t n,
                           float near_, float far_, int probes, int pad, float* bounds, void* stream) {
    const char* fn = "mi_occupancy_clip_rays";
    OccupancyGridArgs grid;
    if (int rc = occupancy_grid_args(fn, bits, dims, lo, inv_cell, &grid)) return rc;
    if (int rc = occupancy_clip_args(fn, near_, far_, probes, pad)) return rc;
    if (n < 0) { set_error("%s: n = %lld", fn, (long long)n); return MI_EINVAL; }
    if (!rays || !bounds) { set_error("%s: null pointer argument (rays, bounds)", fn); return MI_EINVAL; }
    return launch_occupancy_clip_rays(grid, rays, n, near_, far_, probes, pad, bounds, (hipStream_t)stream);
}

// the two list-driven forwards: inference (acts null) and the one that keeps the listed points' layer inputs
static int eval_rays_list_checked(const char* fn, bool train, int kind, const float* packed, const float* rays, const float* z,
                                  int64_t n, int n_samples, const int* list, const int* count, float* raw, float* acts, void* stream) {
    if (bad_kind(kind)) return MI_EINVAL;
    if (!has_list_kernel(kind)) { set_error("%s: kind %d has no list-driven forward (NeRF, SirenNeRF, TinyNeRF have)", fn, kind); return MI_EINVAL; }
    if (!packed || !rays || !z || !list || !count || !raw || (train && !acts)) { set_error("%s: null pointer argument", fn); return MI_EINVAL; }
    if (int rc = check_list_sizes(fn, n, n_samples)) return rc;
    if (n == 0) return MI_OK;
    return eval_rays_list(kind, packed, rays, z, n, n_samples, list, count, raw, acts, (hipStream_t)stream);
}

int mi_field_eval_rays_list(int kind, const float* packed, const float* rays, const float* z, int64_t n, int n_samples,
                            const int* list, const int* count, float* raw, void* stream) {
    return eval_rays_list_checked("mi_field_eval_rays_list", false, kind, packed, rays, z, n, n_samples, list, count, raw, nullptr, stream);
}

int mi_field_eval_rays_list_train(int kind, const float* packed, const float* rays, const float* z, int64_t n, int n_samples,
                                  const int* list, const int* count, float* raw, float* acts, void* stream) {
    return eval_rays_list_checked("mi_field_eval_rays_list_train", true, kind, packed, rays, z, n, n_samples, list, count, raw, acts, stream);
}

int mi_field_backward_list(int kind, const float* packed_bwd, const float* acts, float* grads_ws, const float* raw,
                           const float* g_raw, const int* list, const int* count, int64_t capacity, float* partial_ws,
                           float* const* grad_params, void* stream) {
    const char* fn = "mi_field_backward_list";
    if (bad_kind(kind)) return MI_EINVAL;
    if (!has_list_kernel(kind)) { set_error("%s: kind %d has no counted backward (NeRF, SirenNeRF, TinyNeRF have)", fn, kind); return MI_EINVAL; }
    if (!packed_bwd || !acts || !grads_ws || !raw || !g_raw || !list || !count || !partial_ws || !grad_params) {
        set_error("%s: null pointer argument", fn);
        return MI_EINVAL;
    }
    if (capacity < 0 || capacity > 0x7fffffffLL) { set_error("%s: capacity %lld does not fit the list's int indices", fn, (long long)capacity); return MI_EINVAL; }
    for (int i = 0; i < 2 * field_kind(kind).n_layers; ++i)
        if (!grad_params[i]) { set_error("%s: gradient pointer %d is null", fn, i); return MI_EINVAL; }
    return launch_field_backward_list(kind, packed_bwd, acts, grads_ws, raw, g_raw, list, count, capacity, partial_ws, grad_params,
                                      (hipStream_t)stream);
}

int mi_gen_rays(int width, int height, double focal, const float* c2w_host, int64_t ray0, int64_t n, float* rays,
                int compute_f64, void* stream) {
    if (width <= 0 || height <= 0 || !c2w_host || !rays || ray0 < 0 || n < 0 || ray0 + n > (int64_t)width * height) {
        set_error("mi_gen_rays: bad arguments");
        return MI_EINVAL;
    }
    return launch_gen_rays(width, height, focal, c2w_host, ray0, n, rays, compute_f64, (hipStream_t)stream);
}

int mi_sample_coarse(int64_t n, float near_, float far_, int n_coarse, const float* z_lin, const float* t_rand,
                     uint64_t seed, uint64_t ray0, float* z, void* stream) {
    if (n < 0 || n_coarse < 1 || !z) { set_error("mi_sample_coarse: bad arguments"); return MI_EINVAL; }
    return launch_sample_coarse(n, near_, far_, n_coarse, z_lin, t_rand, seed, ray0, z, (hipStream_t)stream);
}

int mi_sample_coarse_bounds(int64_t n, const float* bounds, int n_coarse, const float* t_rand, uint64_t seed, uint64_t ray0,
                            float* z, void* stream) {
    if (n < 0 || n_coarse < 1 || !bounds || !z) { set_error("mi_sample_coarse_bounds: bad arguments (bounds and z are required)"); return MI_EINVAL; }
    return launch_sample_coarse_bounds(n, bounds, n_coarse, t_rand, seed, ray0, z, (hipStream_t)stream);
}

int mi_composite(int64_t n, int n_samples, const float* raw, const float* z, const float* rays, float* rgb,
                 float* depth, float* acc, float* weights, void* stream) {
    if (n < 0 || n_samples < 1 || !raw || !z || !rays || !rgb || !depth || !acc) {
        set_error("mi_composite: bad arguments");
        return MI_EINVAL;
    }
    return launch_composite(n, n_samples, raw, z, rays, rgb, depth, acc, weights, (hipStream_t)stream);
}

int mi_sample_fine(int64_t n, float near_, float far_, int n_coarse, int n_fine, const float* z_lin,
                   const float* u_lin, const float* z_coarse, const float* weights, float* z_samples, float* z_fine,
                   void* stream) {
    // sample_pdf is called with mids (Nc-1 bins) and weights[1:-1] (Nc-2): needs Nc >= 3
    if (n < 0 || n_coarse < 3 || n_fine < 0 || !z_coarse || !weights || !z_fine) {
        set_error("mi_sample_fine: bad arguments (need Nc >= 3)");
        return MI_EINVAL;
    }
    return launch_sample_fine(n, near_, far_, n_coarse, n_fine, z_lin, u_lin, z_coarse, weights, z_samples, z_fine, nullptr,
                              (hipStream_t)stream);
}

int mi_sample_fine_pos(int64_t n, float near_, float far_, int n_coarse, int n_fine, const float* z_lin,
                       const float* u_lin, const float* z_coarse, const float* weights, float* z_samples, float* z_fine,
                       int* pos, void* stream) {
    if (n < 0 || n_coarse < 3 || n_fine < 0 || !z_coarse || !weights || !z_fine || !pos) {
        set_error("mi_sample_fine_pos: bad arguments (need Nc >= 3 and a pos table)");
        return MI_EINVAL;
    }
    return launch_sample_fine(n, near_, far_, n_coarse, n_fine, z_lin, u_lin, z_coarse, weights, z_samples, z_fine, pos,
                              (hipStream_t)stream);
}

int mi_sample_fine_bounds(int64_t n, const float* bounds, int n_coarse, int n_fine, const float* u_lin, const float* z_coarse,
                          const float* weights, float* z_samples, float* z_fine, int* pos, void* stream) {
    if (n < 0 || n_coarse < 3 || n_fine < 0 || !bounds || !z_coarse || !weights || !z_fine) {
        set_error("mi_sample_fine_bounds: bad arguments (need Nc >= 3 and the bounds)");
        return MI_EINVAL;
    }
    return launch_sample_fine_bounds(n, bounds, n_coarse, n_fine, u_lin, z_coarse, weights, z_samples, z_fine, pos, (hipStream_t)stream);
}

int mi_merge_raw(int64_t n, int n_coarse, int n_fine, const float* raw_coarse, const float* raw_samples, const int* pos,
                 float* raw_fine, void* stream) {
    if (n < 0 || n_coarse < 1 || n_fine < 0 || !raw_coarse || (n_fine > 0 && !raw_samples) || !pos || !raw_fine) {
        set_error("mi_merge_raw: bad arguments");
        return MI_EINVAL;
    }
    return launch_merge_raw(n, n_coarse, n_fine, raw_coarse, raw_samples, pos, raw_fine, (hipStream_t)stream);
}

int mi_split_grad(int64_t n, int n_coarse, int n_fine, const float* g_raw_fine, const int* pos, float* g_raw_coarse,
                  int accumulate_coarse, float* g_raw_samples, void* stream) {
    if (n < 0 || n_coarse < 1 || n_fine < 0 || !g_raw_fine || !pos || !g_raw_coarse || (n_fine > 0 && !g_raw_samples)) {
        set_error("mi_split_grad: bad arguments");
        return MI_EINVAL;
    }
    return launch_split_grad(n, n_coarse, n_fine, g_raw_fine, pos, g_raw_coarse, accumulate_coarse, g_raw_samples,
                             (hipStream_t)stream);
}

int mi_sample_pdf(int64_t n, int n_bins, int n_samples, const float* bins, const float* weights, const float* u_lin,
                  float* samples, void* stream) {
    if (n < 0 || n_bins < 2 || n_samples < 0 || !bins || !weights || (n_samples > 0 && !samples)) {
        set_error("mi_sample_pdf: bad arguments (need at least 2 bins)");
        return MI_EINVAL;
    }
    return launch_sample_pdf(n, n_bins, n_samples, bins, weights, u_lin, samples, (hipStream_t)stream);
}

int mi_composite_bwd(int64_t n, int n_samples, const float* raw, const float* z, const float* rays,
                     const float* g_rgb, const float* g_depth, const float* g_acc, const float* g_weights, float* g_raw,
                     void* stream) {
    if (n < 0 || n_samples < 1 || !raw || !z || !rays || !g_raw) { set_error("mi_composite_bwd: bad arguments"); return MI_EINVAL; }
    return launch_composite_bwd(n, n_samples, raw, z, rays, g_rgb, g_depth, g_acc, g_weights, g_raw, (hipStream_t)stream);
}

int64_t mi_field_packed_bwd_floats(int kind) { return bad_kind(kind) ? MI_EINVAL : packed_floats(field_kind(kind).bwd); }

int mi_field_pack_bwd(int kind, const float* const* params, int n_params, float w_0, float* packed_bwd, void* stream) {
    if (bad_kind(kind)) return MI_EINVAL;
    if (!params || !packed_bwd || n_params != 2 * field_kind(kind).n_layers) { set_error("mi_field_pack_bwd: bad arguments"); return MI_EINVAL; }
    if (int rc = check_w0(kind, w_0, "mi_field_pack_bwd")) return rc;
    return launch_pack(kind, STREAM_BWD, params, n_params, w_0, packed_bwd, (hipStream_t)stream);
}

int64_t mi_field_train_acts_floats(int kind) { return bad_kind(kind) ? MI_EINVAL : region_total(field_kind(kind).acts); }
int64_t mi_field_train_grads_floats(int kind) { return bad_kind(kind) ? MI_EINVAL : region_total(field_kind(kind).grads); }
int64_t mi_field_bwd_partial_floats(int64_t points) { return bwd_partial_floats(points); }
int64_t mi_field_bwd_partial_floats_kind(int kind, int64_t points) { return bad_kind(kind) ? MI_EINVAL : bwd_partial_floats_kind(kind, points); }

int mi_field_eval_rays_train(int kind, const float* packed, const float* film, const float* rays, const float* z,
                             int64_t n_groups, int64_t rays_per_group, int n_samples, float* raw, float* acts,
                             void* stream) {
    if (n_samples <= 0 || !acts) { set_error("mi_field_eval_rays_train: bad arguments"); return MI_EINVAL; }
    if (bad_kind(kind)) return MI_EINVAL;
    return eval_common(kind, packed, film, rays, z, n_groups, rays_per_group * n_samples, rays_per_group, n_samples, 1,
                       raw, (hipStream_t)stream, acts);
}

int mi_field_eval_points_train(int kind, const float* packed, const float* film, const float* x, int64_t n_groups,
                               int64_t points_per_group, float* out, float* acts, void* stream) {
    if (!acts) { set_error("mi_field_eval_points_train: bad arguments"); return MI_EINVAL; }
    if (bad_kind(kind)) return MI_EINVAL;
    return eval_common(kind, packed, film, x, nullptr, n_groups, points_per_group, 0, 1, 0, out, (hipStream_t)stream, acts);
}

int64_t mi_field_film_partial_floats(int64_t n_groups, int64_t points_per_group) {
    return film_partial_floats(n_groups, points_per_group);
}

int64_t mi_field_film_partial_floats_kind(int kind, int64_t n_groups, int64_t points_per_group) {
    return bad_kind(kind) ? MI_EINVAL : film_partial_floats_kind(kind, n_groups, points_per_group);
}

int mi_field_backward(int kind, const float* packed_bwd, const float* film, const float* acts, float* grads_ws,
                      const float* raw, const float* g_raw, int64_t n_groups, int64_t points_per_group,
                      float* partial_ws, float* film_partial_ws, float* const* grad_params,
                      const float* const* params, int n_params, float* grad_film, void* stream) {
    if (bad_kind(kind)) return MI_EINVAL;
    if (!packed_bwd || !acts || !grads_ws || !raw || !g_raw || !partial_ws || !grad_params ||
        n_params != 2 * field_kind(kind).n_layers) { set_error("mi_field_backward: bad arguments"); return MI_EINVAL; }
    const bool film_kind = is_film(kind);
    for (int i = 0; i < n_params; ++i) {
        if (!grad_params[i]) { set_error("gradient pointer %d is null", i); return MI_EINVAL; }
        if (film_kind && (!params || !params[i])) { set_error("FiLM kinds need parameter pointer %d", i); return MI_EINVAL; }
    }
    return launch_field_backward(kind, packed_bwd, acts, grads_ws, raw, g_raw, n_groups, points_per_group, film,
                                 film_partial_ws, grad_film, partial_ws, grad_params, params, (hipStream_t)stream);
}

// shared argument checks of the two input-gradient calls
static int check_input_grad(const char* fn, int kind, const float* const* params, int n_params, const float* film,
                            const float* acts, const float* grads_ws, int64_t n_groups, int64_t per_group, const float* out) {
    if (bad_kind(kind)) return MI_EINVAL;
    if (!params || !acts || !grads_ws || !out) { set_error("%s: null pointer argument", fn); return MI_EINVAL; }
    if (n_params != 2 * field_kind(kind).n_layers) {
        set_error("%s: kind %d expects %d parameter tensors, got %d", fn, kind, 2 * field_kind(kind).n_layers, n_params);
        return MI_EINVAL;
    }
    for (int i = 0; i < n_params; ++i)
        if (!params[i]) { set_error("%s: parameter %d is null", fn, i); return MI_EINVAL; }
    if (is_film(kind) && !film) { set_error("%s: FiLM kind needs a film table", fn); return MI_EINVAL; }
    if (n_groups < 0 || per_group < 0) { set_error("%s: negative size", fn); return MI_EINVAL; }
    if (!is_film(kind) && n_groups > 1) { set_error("%s: only FiLM kinds have groups (n_groups = %lld)", fn, (long long)n_groups); return MI_EINVAL; }
    return MI_OK;
}

int mi_field_input_grad(int kind, const float* const* params, int n_params, const float* film, const float* acts,
                        const float* grads_ws, int64_t n_groups, int64_t points_per_group, float* g_x, void* stream) {
    if (int rc = check_input_grad("mi_field_input_grad", kind, params, n_params, film, acts, grads_ws, n_groups,
                                  points_per_group, g_x)) return rc;
    return launch_field_input_grad(kind, params, film, acts, grads_ws, n_groups, points_per_group, g_x, (hipStream_t)stream);
}

int mi_field_input_grad_rays(int kind, const float* const* params, int n_params, const float* film, const float* acts,
                             const float* grads_ws, const float* rays, const float* z, int64_t n_groups,
                             int64_t rays_per_group, int n_samples, int accumulate, float* g_rays, void* stream) {
    if (int rc = check_input_grad("mi_field_input_grad_rays", kind, params, n_params, film, acts, grads_ws, n_groups,
                                  rays_per_group, g_rays)) return rc;
    if (!rays || !z) { set_error("mi_field_input_grad_rays: null pointer argument"); return MI_EINVAL; }
    if (n_samples < 1) { set_error("mi_field_input_grad_rays: n_samples must be positive"); return MI_EINVAL; }
    return launch_field_input_grad_rays(kind, params, film, acts, grads_ws, rays, z, n_groups, rays_per_group, n_samples,
                                        accumulate, g_rays, (hipStream_t)stream);
}

int mi_field_input_grad_rays_list(int kind, const float* const* params, int n_params, const float* acts, const float* grads_ws,
                                  const int* list, const int* count, int64_t capacity, const float* rays, const float* z,
                                  int64_t n, int n_samples, int accumulate, float* g_rays, void* stream) {
    const char* fn = "mi_field_input_grad_rays_list";
    if (bad_kind(kind)) return MI_EINVAL;
    if (!has_list_kernel(kind)) { set_error("%s: kind %d has no counted backward (NeRF, SirenNeRF, TinyNeRF have)", fn, kind); return MI_EINVAL; }
    if (int rc = check_input_grad(fn, kind, params, n_params, nullptr, acts, grads_ws, 1, n, g_rays)) return rc;
    if (!list || !count || !rays || !z) { set_error("%s: null pointer argument", fn); return MI_EINVAL; }
    if (n_samples < 1) { set_error("%s: n_samples must be positive", fn); return MI_EINVAL; }
    if (n > 0x7fffffffLL / n_samples) {
        set_error("%s: n * n_samples = %lld * %d exceeds 2^31 - 1 (the list holds int point indices)", fn, (long long)n, n_samples);
        return MI_EINVAL;
    }
    if (capacity != n * n_samples) {
        set_error("%s: capacity %lld is not n * n_samples = %lld (the stride of the compact regions)", fn, (long long)capacity,
                  (long long)(n * n_samples));
        return MI_EINVAL;
    }
    return launch_field_input_grad_rays_list(kind, params, acts, grads_ws, list, count, rays, z, n, n_samples, accumulate, g_rays,
                                             (hipStream_t)stream);
}

int mi_composite_bwd_rays(int64_t n, int n_samples, const float* raw, const float* z, const float* rays,
                          const float* g_rgb, const float* g_depth, const float* g_acc, const float* g_weights,
                          int accumulate, float* g_rays, void* stream) {
    if (n < 0 || n_samples < 1 || n_samples > 4096 || !raw || !z || !rays || !g_rays) {
        set_error("mi_composite_bwd_rays: bad arguments (non-null raw, z, rays, g_rays; 1 <= n_samples <= 4096)");
        return MI_EINVAL;
    }
    return launch_composite_bwd_rays(n, n_samples, raw, z, rays, g_rgb, g_depth, g_acc, g_weights, accumulate, g_rays,
                                     (hipStream_t)stream);
}

#ifdef MI_PROFILE_STAMPS
void mi_debug_set_stamps(void* p) { g_stamps = (unsigned long long*)p; g_bwd_stamps = (unsigned long long*)p; }
#endif

int64_t mi_image_metrics_workspace_floats(int images, int channels, int height, int width) {
    if (images <= 0 || channels <= 0 || height <= 0 || width <= 0) return 0;
    return image_metrics_workspace_floats(images, channels, height, width);
}

int mi_image_metrics(const float* img1, const float* img2, int images, int channels, int height, int width,
                     const float* window, int window_size, float* workspace, float* out, void* stream) {
    if (!img1 || !img2 || !window || !workspace || !out || images <= 0 || channels <= 0 || height <= 0 || width <= 0 ||
        window_size < 1 || window_size > 31 || window_size % 2 == 0) {
        set_error("mi_image_metrics: bad arguments (window must be odd and <= 31)");
        return MI_EINVAL;
    }
    return launch_image_metrics(img1, img2, images, channels, height, width, window, window_size, workspace, out,
                                (hipStream_t)stream);
}

int mi_grid_points(int n, const float* voxel_origin, float voxel_size, int64_t head, int64_t count, float* points,
                   void* stream) {
    if (n <= 0 || !voxel_origin || head < 0 || count < 0 || head + count > (int64_t)n * n * n || (count > 0 && !points)) {
        set_error("mi_grid_points: bad arguments (need 0 <= head, head + count <= n^3)");
        return MI_EINVAL;
    }
    return launch_grid_points(n, voxel_origin, voxel_size, head, count, points, (hipStream_t)stream);
}

int64_t mi_nerf_loss_workspace_floats(int64_t n) { return n > 0 ? nerf_loss_workspace_floats(n) : 0; }

int mi_nerf_loss(int64_t n, const float* rgb_c, const float* acc_c, const float* rgb_f, const float* acc_f,
                 const float* target, int use_alpha, int use_fine_model, float* g_rgb_c, float* g_acc_c, float* g_rgb_f,
                 float* g_acc_f, float* workspace, float* out, void* stream) {
    if (n <= 0 || !rgb_c || !acc_c || !rgb_f || !acc_f || !target || !g_rgb_c || !g_acc_c || !g_rgb_f || !g_acc_f ||
        !workspace || !out) { set_error("mi_nerf_loss: bad arguments"); return MI_EINVAL; }
    return launch_nerf_loss(n, rgb_c, acc_c, rgb_f, acc_f, target, use_alpha, use_fine_model, g_rgb_c, g_acc_c, g_rgb_f,
                            g_acc_f, workspace, out, (hipStream_t)stream);
}

int mi_ray_bank(int width, int height, double focal, const float* poses, const float* rgba, int white_bkgd, int64_t images,
                float* rays_rgba, int compute_f64, void* stream) {
    if (width <= 0 || height <= 0 || images < 0 || !poses || !rgba || (images > 0 && !rays_rgba)) {
        set_error("mi_ray_bank: bad arguments");
        return MI_EINVAL;
    }
    return launch_ray_bank(width, height, focal, poses, rgba, white_bkgd, images, rays_rgba, compute_f64, (hipStream_t)stream);
}

int mi_adam_step(int n_fields, const int* kinds, float* const* params, const float* const* grads, float* const* exp_avg,
                 float* const* exp_avg_sq, const int64_t* numel, float step_size, float one_minus_beta1, float beta2,
                 float one_minus_beta2, float eps, float bias_correction2_sqrt, float* const* packed_fwd,
                 float* const* packed_bwd, void* stream) {
    if (n_fields < 1 || n_fields > 2 || !kinds || !params || !grads || !exp_avg || !exp_avg_sq || !numel || !packed_fwd) {
        set_error("mi_adam_step: bad arguments (1 or 2 fields, non-null tables)");
        return MI_EINVAL;
    }
    int n_params[2] = {0, 0}, total = 0;
    for (int f = 0; f < n_fields; ++f) {
        if (bad_kind(kinds[f])) return MI_EINVAL;
        if (!packed_fwd[f]) { set_error("mi_adam_step: field %d has no packed stream", f); return MI_EINVAL; }
        n_params[f] = 2 * field_kind(kinds[f]).n_layers;
        total += n_params[f];
    }
    for (int t = 0; t < total; ++t)
        if (!params[t] || !grads[t] || !exp_avg[t] || !exp_avg_sq[t] || numel[t] < 0) {
            set_error("mi_adam_step: tensor %d has a null pointer", t);
            return MI_EINVAL;
        }
    return launch_adam_step(n_fields, kinds, n_params, params, grads, exp_avg, exp_avg_sq, numel, step_size, one_minus_beta1,
                            beta2, one_minus_beta2, eps, bias_correction2_sqrt, packed_fwd, packed_bwd, (hipStream_t)stream);
}

void* mi_event_create(void) {
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) { set_error("hipEventCreate failed"); return nullptr; }
    return (void*)e;
}
void mi_event_destroy(void* ev) { if (ev) (void)hipEventDestroy((hipEvent_t)ev); }
int mi_event_record(void* ev, void* stream) {
    if (hipEventRecord((hipEvent_t)ev, (hipStream_t)stream) != hipSuccess) { set_error("hipEventRecord failed"); return MI_EHIP; }
    return MI_OK;
}
int mi_event_elapsed_ms(void* start, void* stop, float* ms) {
    if (hipEventSynchronize((hipEvent_t)stop) != hipSuccess ||
        hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop) != hipSuccess) {
        set_error("hipEventElapsedTime failed");
        return MI_EHIP;
    }
    return MI_OK;
}

}  // extern "C"
