// occupancy_path.hip - rendering and training with an occupancy grid through the C ABI (include/mi_render.h):
// mi_render_rays_occupancy, mi_render_rays_occupancy_train, mi_render_rays_occupancy_backward (and its _rays form, which also
// gives dL/d(rays): occupancy_backward) and their size queries.
// The forwards are one body (occupancy_render) over one struct of their arguments (OccArgs).  It runs the sequence of every render
// path (run_render_passes, render_path.h) with one field step (occupancy_forward):
// per pass, mark the samples in occupied cells into a device-counted list and evaluate the field at the listed points alone.
// Training differs in three values: the ordered mark, a field that keeps the listed points' layer inputs, and a list per pass
// (OccLists), which the backward reads.  The grid checks of every call that reads one (occupancy_grid_args) and the list-driven
// field launch (eval_rays_list) are here too, for the stage wrappers of api.hip as well.  It is deliberately small:
// one range per pass, nothing recomputed, one group, no FiLM; one field for both passes runs as two passes of that field over
// all their listed points (no merge, as at inference) and its two gradient sums are added.
// The clipped forwards (mi_render_rays_occupancy_clip / _clip_train) are the same body with one launch in front: each
// ray's range clipped to the grid (launch_occupancy_clip_rays) into a bounds region behind the lists, which both samplers read.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "render_path.h"

namespace mi {

// dims >= 1 with a product below 2^31 (a cell's bit index is an int); the product, or 0 with the error set
int64_t occupancy_cells(const char* fn, const int* dims) {
    if (!dims) { set_error("%s: null grid dims", fn); return 0; }
    int64_t cells = 1;
    for (int c = 0; c < 3; ++c) {
        if (dims[c] < 1) { set_error("%s: grid dims %d x %d x %d (each must be at least 1)", fn, dims[0], dims[1], dims[2]); return 0; }
        cells *= dims[c];                                  // < 2^31 * 2^31 before the check below
        if (cells >= (int64_t)1 << 31) { set_error("%s: grid dims %d x %d x %d (2^31 cells or more)", fn, dims[0], dims[1], dims[2]); return 0; }
    }
    return cells;
}

// the one place a grid is checked: its dims first, then its three pointers
int occupancy_grid_args(const char* fn, const uint32_t* bits, const int* dims, const float* lo, const float* inv_cell,
                        OccupancyGridArgs* grid) {
    if (!occupancy_cells(fn, dims)) return MI_EINVAL;
    if (!bits || !lo || !inv_cell) { set_error("%s: null pointer argument", fn); return MI_EINVAL; }
    for (int d = 0; d < 3; ++d) { grid->cells.dims[d] = dims[d]; grid->cells.lo[d] = lo[d]; grid->cells.inv_cell[d] = inv_cell[d]; }
    grid->bits = bits;
    return MI_OK;
}

// the field at the points of a device-counted list: a mode-1 launch of one group of n rays x S samples; acts: the listed
// points' layer inputs are kept there (training), null = inference
int eval_rays_list(int kind, const float* packed, const float* rays, const float* z, int64_t n, int S, const int* list,
                   const int* count, float* raw, float* acts, hipStream_t hs) {
    MlpArgs args = {};
    args.packed = packed; args.a = rays; args.z = z; args.out = raw;
    args.points_per_group = n * S; args.rays_per_group = n; args.tiles_per_group = (n * S + 127) / 128;
    args.n_samples = S; args.mode = 1; args.save = acts; args.save_points = n * S; args.n_rays = n;
    return launch_mlp_list(kind, args, list, count, hs);
}

// The region behind RenderWorkspace::base_bytes(), in ints, each part on a 64-int block.  Inference: one list of n (Nc + Nf)
// ints that the passes fill in turn.  Training: an ascending list per pass, each with its scan slots
// (occupancy_ordered_list_ints).  Then the two counts.
struct OccLists {
    struct Regions { int* list[2]; int* counts; };
    int64_t ints[2];                                     // ints[1] == 0: the fine pass reuses the coarse pass's list
    OccLists(bool training, int64_t n, int nc, int nf) {
        const int64_t pc = n * nc, pf = n * ((int64_t)nc + nf);
        ints[0] = align64(training ? occupancy_ordered_list_ints(pc) : pf);
        ints[1] = training ? align64(occupancy_ordered_list_ints(pf)) : 0;
    }
    int64_t bytes() const { return (ints[0] + ints[1] + align64(2)) * (int64_t)sizeof(int); }
    Regions carve(const void* workspace, int64_t base_bytes) const {
        int* first = (int*)((char*)const_cast<void*>(workspace) + base_bytes);
        return {{first, ints[1] ? first + ints[0] : first}, first + ints[0] + ints[1]};
    }
};

// near_ < far_ (so neither is a NaN), 1 <= probes <= 4096 (64 rounds of a wave), pad >= 0
int occupancy_clip_args(const char* fn, float near_, float far_, int probes, int pad) {
    if (!(near_ < far_)) { set_error("%s: near = %g, far = %g (clipping needs near < far)", fn, (double)near_, (double)far_); return MI_EINVAL; }
    if (probes < 1 || probes > 4096) { set_error("%s: probes = %d (1 to 4096)", fn, probes); return MI_EINVAL; }
    if (pad < 0) { set_error("%s: pad = %d (at least 0)", fn, pad); return MI_EINVAL; }
    return MI_OK;
}

// The bounds [n,2] of a clipped call (mi_render_occupancy_clip_extra_bytes): behind the OccLists region of either kind, so
// every offset the backward reads stays where it is without them.
static int64_t clip_bounds_bytes(int64_t n) { return align64(2 * n) * (int64_t)sizeof(float); }

// the backward workspace, in floats: dL/d(raw) of both composites, one pass's dA rows and dW scratch, one field: the fine
// pass's parameter gradients
struct OccBwdLayout {
    int64_t g_raw_c, g_raw_f, grads, partial, fine_total, total;
    OccBwdLayout(int kind_c, int kind_f, bool shared, int64_t n, int nc, int nf) {
        const int64_t pc = n * nc, pf = n * ((int64_t)nc + nf);
        RegionAllocator ws;
        const int64_t gc = pc * region_total(field_kind(kind_c).grads), gf = pf * region_total(field_kind(kind_f).grads);
        const int64_t bc = bwd_partial_floats_kind(kind_c, pc), bf = bwd_partial_floats_kind(kind_f, pf);
        g_raw_c = ws.take(pc * 4);
        g_raw_f = ws.take(pf * 4);
        grads = ws.take(gc > gf ? gc : gf);
        partial = ws.take(bc > bf ? bc : bf);
        fine_total = ws.take(shared ? param_floats(kind_c) : 0);
        total = ws.floats;
    }
    int64_t bytes() const { return total * (int64_t)sizeof(float); }
};

// the compact saved rows of the coarse pass; the fine pass's follow them
static int64_t saved_floats_coarse(int kind_c, int64_t n, int nc) { return region_total(field_kind(kind_c).acts) * n * nc; }
static int64_t saved_bytes_of(int kind_c, int kind_f, int64_t n, int nc, int nf) {
    return 4 * (saved_floats_coarse(kind_c, n, nc) + region_total(field_kind(kind_f).acts) * n * ((int64_t)nc + nf));
}

// Sizes, kinds, the list kernels, the int bound on a pass's points and - where the call reads one (grid non-null) - the grid.
// doing: "rendering" / "training", the word in which the two calls' FiLM messages differ.
static int check_call(const char* fn, const char* doing, int kind_c, int kind_f, int64_t n, int nc, int nf, const uint32_t* bits = nullptr,
                      const int* dims = nullptr, const float* lo = nullptr, const float* inv_cell = nullptr, OccupancyGridArgs* grid = nullptr) {
    if (n < 0 || nc < 3 || nf < 0) { set_error("%s: bad sizes (n >= 0, Nc >= 3, Nf >= 0)", fn); return MI_EINVAL; }
    if (bad_kind(kind_c) || bad_kind(kind_f)) return MI_EINVAL;
    if (!has_list_kernel(kind_c) || !has_list_kernel(kind_f)) {
        set_error("%s: kinds %d / %d: %s with a grid is built for NeRF, SirenNeRF and TinyNeRF, not for FiLM kinds", fn, kind_c, kind_f, doing);
        return MI_EINVAL;
    }
    if (n > 0x7fffffffLL / (nc + nf)) {
        set_error("%s: n * (Nc + Nf) = %lld * %d exceeds 2^31 - 1 (the list holds int point indices)", fn, (long long)n, nc + nf);
        return MI_EINVAL;
    }
    return grid ? occupancy_grid_args(fn, bits, dims, lo, inv_cell, grid) : MI_OK;
}

// The arguments of a grid-driven call, in the order in which the four forwards' extern "C" signatures name them (z_lin: null
// in a clipped call, which takes probes and pad in its place; saved: the training forwards alone).  The backward fills in
// what check_buffers reads: the kinds, the sizes, the workspace and the saved rows.
struct OccArgs {
    int kind_c; const float* packed_c; int kind_f; const float* packed_f;
    const float* rays; int64_t n; float near_, far_; int nc, nf;
    const float *z_lin, *u_lin, *t_rand; uint64_t seed, ray0;
    const uint32_t* bits; const int* dims; const float *lo, *inv_cell;
    float *rgb_c, *depth_c, *acc_c, *rgb_f, *depth_f, *acc_f; int* evaluated;
    void* workspace; int64_t workspace_bytes; void* saved; int64_t saved_bytes;
    void* stream;
};

// The caller's buffers against the size queries: the workspace always, the saved rows from the training forward on, the
// backward workspace (with `shared`, which sizes it) in the backward.
enum OccCall { OCC_RENDER, OCC_TRAIN, OCC_BACKWARD };
static int check_buffers(const char* fn, OccCall call, const OccArgs& a, bool clipped, bool shared = false,
                         const void* bwd_workspace = nullptr, int64_t bwd_workspace_bytes = 0) {
    const auto refused = [&](const char* what, const void* p, int64_t have, int64_t need, const char* query) {
        if (p && have >= need) return false;
        set_error("%s: %s of %lld bytes, %s %lld", fn, what, (long long)have, query, (long long)need);
        return true;
    };
    const bool train = call != OCC_RENDER;
    // A workspace may be larger than asked for: the backward of a clipped forward gets the forward's, bounds region included.
    if (refused("workspace", a.workspace, a.workspace_bytes,
                RenderWorkspace(a.n, a.nc, a.nf).base_bytes() + OccLists(train, a.n, a.nc, a.nf).bytes() + (clipped ? clip_bounds_bytes(a.n) : 0),
                clipped ? (train ? "mi_render_workspace_bytes + mi_render_occupancy_train_extra_bytes + mi_render_occupancy_clip_extra_bytes say"
                                 : "mi_render_workspace_bytes + mi_render_occupancy_extra_bytes + mi_render_occupancy_clip_extra_bytes say")
                : train ? "mi_render_workspace_bytes + mi_render_occupancy_train_extra_bytes say"
                        : "mi_render_workspace_bytes + mi_render_occupancy_extra_bytes say") ||
        (train && refused("saved buffer", a.saved, a.saved_bytes, saved_bytes_of(a.kind_c, a.kind_f, a.n, a.nc, a.nf),
                          "mi_render_occupancy_train_saved_bytes says")) ||
        (call == OCC_BACKWARD && refused("backward workspace", bwd_workspace, bwd_workspace_bytes,
                                         OccBwdLayout(a.kind_c, a.kind_f, shared, a.n, a.nc, a.nf).bytes(),
                                         "mi_render_occupancy_backward_workspace_bytes says")))
        return MI_EINVAL;
    return MI_OK;
}

// Refuses grid words that the runtime knows as memory of ANOTHER device; what it cannot classify is left to the launch.
static int check_grid_device(const char* fn, const uint32_t* bits) {
    hipPointerAttribute_t attr;
    int dev = 0;
    if (hipPointerGetAttributes(&attr, bits) != hipSuccess || hipGetDevice(&dev) != hipSuccess) {
        (void)hipGetLastError();
        return MI_OK;
    }
    if (attr.type == hipMemoryTypeDevice && attr.device != dev) {
        set_error("%s: the occupancy grid is on device %d, the call runs on device %d", fn, attr.device, dev);
        return MI_EINVAL;
    }
    return MI_OK;
}

// one pass of the sequence: its field, where its list and count go, and where the listed points' layer inputs go (null: inference)
struct OccPass { int kind; const float* packed; int* list; int* count; float* acts; };

// The grid-driven forward: the sequence of every render path, always with the whole fine pass (one field runs as two passes of
// that field, Nf = 0 included), its field step = mark, then the list-driven field; then the copy of the two counts.  Everything is
// already checked.  ordered: the ascending mark that training needs.  Without io.rgb_c the coarse composite gives the weights alone.
// clip (null: none): first the clip of every ray's range to the grid into `bounds`, which the sequence's samplers then read in
// place of io's near_ / far_ / z_lin - a launch in front, no read-back.
struct OccClip { int probes, pad; float* bounds; };

static int occupancy_forward(const char* fn, const OccPass pass[2], bool ordered, const OccupancyGridArgs& grid, int64_t n, int nc,
                             int nf, RenderIO io, const OccClip* clip, int* evaluated, const RenderWorkspace::Regions& ws,
                             hipStream_t hs) {
    if (clip) {
        if (int rc = launch_occupancy_clip_rays(grid, io.rays, n, io.near_, io.far_, clip->probes, clip->pad, clip->bounds, hs)) return rc;
        io.bounds = clip->bounds;
    }
    const auto field = [&](const OccPass& p) {
        return [&, p](const float* z, int samples, float* raw) -> int {
            const auto mark = ordered ? launch_occupancy_mark_rays_ordered : launch_occupancy_mark_rays;
            if (int rc = mark(grid, io.rays, z, n, samples, p.list, p.count, raw, hs)) return rc;
            return eval_rays_list(p.kind, p.packed, io.rays, z, n, samples, p.list, p.count, raw, p.acts, hs);
        };
    };
    if (int rc = run_render_passes(fn, RenderCall(1, n, nc, nf, false), FINE_WHOLE, io, ws, COARSE_RAW, field(pass[0]), field(pass[1]), hs))
        return rc;
    // the two counts are neighbours in the workspace (OccLists)
    if (evaluated && hipMemcpyAsync(evaluated, pass[0].count, 2 * sizeof(int), hipMemcpyDeviceToDevice, hs) != hipSuccess) {
        set_error("%s: copy of the evaluated counts failed", fn);
        return MI_EHIP;
    }
    return MI_OK;
}

// What the clipped calls check on top of their unclipped selves: the clip's own arguments (a z_lin table has no meaning per
// ray: they take none).  clip->bounds is set by the caller once the workspace is checked.
static int check_clip(const char* fn, const OccClip* clip, float near_, float far_) {
    return clip ? occupancy_clip_args(fn, near_, far_, clip->probes, clip->pad) : MI_OK;
}

// The four grid-driven forwards: mi_render_rays_occupancy (OCC_RENDER) and mi_render_rays_occupancy_train (OCC_TRAIN), each
// with `clip` as its _clip form.  Inference takes the coarse outputs as optional and leaves a grid on another device to the
// launch; training demands all six outputs and the saved rows, marks in ascending order and keeps the listed points' layer inputs.
static int occupancy_render(const char* fn, OccCall call, OccClip* clip, const OccArgs& a) {
    const bool train = call == OCC_TRAIN;
    OccupancyGridArgs grid;
    if (int rc = check_call(fn, train ? "training" : "rendering", a.kind_c, a.kind_f, a.n, a.nc, a.nf, a.bits, a.dims, a.lo, a.inv_cell, &grid)) return rc;
    if (int rc = check_clip(fn, clip, a.near_, a.far_)) return rc;
    // inference: the coarse outputs are optional, as in mi_render_rays: without rgb_c, depth_c / acc_c each may be null too.
    // Its null workspace is refused here; training's by check_buffers, behind the n == 0 return.
    const bool missing = train ? !a.rgb_c || !a.depth_c || !a.acc_c : !a.workspace || (a.rgb_c && (!a.depth_c || !a.acc_c));
    if (!a.packed_c || !a.packed_f || !a.rays || missing || !a.rgb_f || !a.depth_f || !a.acc_f) {
        set_error("%s: null pointer argument", fn);
        return MI_EINVAL;
    }
    if (a.n == 0) return MI_OK;                                // no rays: nothing to launch, no buffer is touched
    if (int rc = check_buffers(fn, call, a, clip != nullptr)) return rc;
    // Training only: a step is one call, so one host query per step.  Inference renders a frame in many chunks and would pay
    // the query per chunk; nobody has measured that, so mi_render_rays_occupancy leaves a grid on another device to the launch.
    if (train) if (int rc = check_grid_device(fn, a.bits)) return rc;
    const RenderWorkspace layout(a.n, a.nc, a.nf);
    const OccLists lists(train, a.n, a.nc, a.nf);
    const OccLists::Regions r = lists.carve(a.workspace, layout.base_bytes());
    if (clip) clip->bounds = (float*)((char*)a.workspace + layout.base_bytes() + lists.bytes());
    float* acts_c = train ? (float*)a.saved : nullptr;
    float* acts_f = train ? acts_c + saved_floats_coarse(a.kind_c, a.n, a.nc) : nullptr;
    const OccPass pass[2] = {{a.kind_c, a.packed_c, r.list[0], r.counts, acts_c}, {a.kind_f, a.packed_f, r.list[1], r.counts + 1, acts_f}};
    const RenderIO io{a.rays, a.near_, a.far_, a.z_lin, a.u_lin, a.t_rand, a.seed, a.ray0, a.rgb_c, a.depth_c, a.acc_c, a.rgb_f, a.depth_f, a.acc_f};
    return occupancy_forward(fn, pass, train, grid, a.n, a.nc, a.nf, io, clip, a.evaluated, layout.carve(a.workspace), (hipStream_t)a.stream);
}

// a field whose input gradient a backward computes has its parameter tensors (device pointers, state-dict order), every one
static int check_field_params(const char* fn, const char* which, int kind, const float* const* params, int n_params) {
    if (!params) { set_error("%s: null pointer argument (the %s field's parameters)", fn, which); return MI_EINVAL; }
    if (n_params != 2 * field_kind(kind).n_layers) {
        set_error("%s: the %s field's kind %d expects %d parameter tensors, got %d", fn, which, kind, 2 * field_kind(kind).n_layers, n_params);
        return MI_EINVAL;
    }
    for (int i = 0; i < n_params; ++i)
        if (!params[i]) { set_error("%s: parameter %d of the %s field is null", fn, i, which); return MI_EINVAL; }
    return MI_OK;
}

// The backward of both training forwards, stated once: mi_render_rays_occupancy_backward and, with g_rays, its _rays form.
// Per pass with a cotangent: the composite's backward, then the field's over the pass's list.  g_rays (null: no ray output, and
// then not one launch more) is zeroed first and receives, in autograd._RenderRaysFn.backward's order, each composite's |d| part
// over the full raw (an unlisted sample's sigma = 0 gives an exact 0) and each field's input gradient over its list - launched
// right behind that field's backward, whose dA rows in L.grads the next pass overwrites.
static int occupancy_backward(const char* fn, int kind_coarse, const float* packed_bwd_coarse, int kind_fine,
                              const float* packed_bwd_fine, int shared, const float* rays, int64_t n, int n_coarse, int n_fine,
                              const void* workspace, int64_t workspace_bytes, const void* saved, int64_t saved_bytes,
                              const float* g_rgb_c, const float* g_depth_c, const float* g_acc_c, const float* g_rgb_f,
                              const float* g_depth_f, const float* g_acc_f, float* const* grad_params_coarse,
                              float* const* grad_params_fine, void* bwd_workspace, int64_t bwd_workspace_bytes, int* fields_written,
                              const float* const* params_coarse, int n_params_coarse, const float* const* params_fine,
                              int n_params_fine, float* g_rays, void* stream) {
    if (fields_written) *fields_written = 0;
    if (int rc = check_call(fn, "training", kind_coarse, kind_fine, n, n_coarse, n_fine)) return rc;
    if (shared && kind_coarse != kind_fine) { set_error("%s: one field for both passes has one kind (%d and %d)", fn, kind_coarse, kind_fine); return MI_EINVAL; }
    if (n == 0) return MI_OK;
    const bool want_c = g_rgb_c || g_depth_c || g_acc_c, want_f = g_rgb_f || g_depth_f || g_acc_f;
    if (!rays) { set_error("%s: null pointer argument", fn); return MI_EINVAL; }
    const float* const* params[2] = {params_coarse, shared ? params_coarse : params_fine};
    const int n_params[2] = {n_params_coarse, shared ? n_params_coarse : n_params_fine};
    const int kinds[2] = {kind_coarse, kind_fine};
    const float* packed_bwd[2] = {packed_bwd_coarse, shared ? packed_bwd_coarse : packed_bwd_fine};
    float* const* grads[2] = {grad_params_coarse, shared ? grad_params_coarse : grad_params_fine};
    const bool wants[2] = {want_c, want_f};
    for (int f = 0; f < 2; ++f) {
        if (!wants[f]) continue;
        if (int rc = check_field_grads(fn, f && !shared ? "fine" : "coarse", kinds[f], packed_bwd[f], grads[f])) return rc;
        if (g_rays) if (int rc = check_field_params(fn, f && !shared ? "fine" : "coarse", kinds[f], params[f], n_params[f])) return rc;
    }
    OccArgs a = {};
    a.kind_c = kind_coarse; a.kind_f = kind_fine; a.n = n; a.nc = n_coarse; a.nf = n_fine;
    a.workspace = const_cast<void*>(workspace); a.workspace_bytes = workspace_bytes;
    a.saved = const_cast<void*>(saved); a.saved_bytes = saved_bytes;
    if (int rc = check_buffers(fn, OCC_BACKWARD, a, false, shared != 0, bwd_workspace, bwd_workspace_bytes)) return rc;
    hipStream_t hs = (hipStream_t)stream;
    // g_rays = 0 ahead of the launches that add to it, by a kernel (render_stages.hip: a captured memset of these n * 24 bytes
    // did not clear them on replay - tests/test_gpu_graph_occupancy.py, the pose cases)
    if (g_rays) if (int rc = launch_clear_floats(n * 6, g_rays, hs)) return rc;
    if (!want_c && !want_f) return MI_OK;
    const OccBwdLayout L(kind_coarse, kind_fine, shared != 0, n, n_coarse, n_fine);
    const RenderWorkspace layout(n, n_coarse, n_fine);
    const RenderWorkspace::Regions ws = layout.carve(const_cast<void*>(workspace));
    const OccLists::Regions r = OccLists(true, n, n_coarse, n_fine).carve(workspace, layout.base_bytes());
    const float* acts_c = (const float*)saved;
    const float* acts_f = acts_c + saved_floats_coarse(kind_coarse, n, n_coarse);
    const int S = n_coarse + n_fine;
    float* bws = (float*)bwd_workspace;
    int rc;
    if (want_c) {
        if ((rc = launch_composite_bwd(n, n_coarse, ws.raw_c, ws.z_c, rays, g_rgb_c, g_depth_c, g_acc_c, nullptr, bws + L.g_raw_c, hs))) return rc;
        if (g_rays && (rc = launch_composite_bwd_rays(n, n_coarse, ws.raw_c, ws.z_c, rays, g_rgb_c, g_depth_c, g_acc_c, nullptr, 1, g_rays, hs))) return rc;
        if ((rc = launch_field_backward_list(kind_coarse, packed_bwd_coarse, acts_c, bws + L.grads, ws.raw_c, bws + L.g_raw_c, r.list[0],
                                             r.counts, n * n_coarse, bws + L.partial, grad_params_coarse, hs))) return rc;
        if (g_rays && (rc = launch_field_input_grad_rays_list(kind_coarse, params[0], acts_c, bws + L.grads, r.list[0], r.counts, rays, ws.z_c,
                                                              n, n_coarse, 1, g_rays, hs))) return rc;
    }
    if (want_f) {
        if ((rc = launch_composite_bwd(n, S, ws.raw_f, ws.z_f, rays, g_rgb_f, g_depth_f, g_acc_f, nullptr, bws + L.g_raw_f, hs))) return rc;
        if (g_rays && (rc = launch_composite_bwd_rays(n, S, ws.raw_f, ws.z_f, rays, g_rgb_f, g_depth_f, g_acc_f, nullptr, 1, g_rays, hs))) return rc;
        float* fine_total[2 * kMaxLayers];
        const bool add = shared && want_c;                       // one field: coarse-pass total += fine-pass total
        if (add) scratch_params(kind_fine, bws + L.fine_total, fine_total);
        if ((rc = launch_field_backward_list(kind_fine, packed_bwd[1], acts_f, bws + L.grads, ws.raw_f, bws + L.g_raw_f, r.list[1],
                                             r.counts + 1, n * S, bws + L.partial, add ? fine_total : grads[1], hs))) return rc;
        if (g_rays && (rc = launch_field_input_grad_rays_list(kind_fine, params[1], acts_f, bws + L.grads, r.list[1], r.counts + 1, rays, ws.z_f,
                                                              n, S, 1, g_rays, hs))) return rc;
        if (add && (rc = add_param_grads(kind_fine, grad_params_coarse, fine_total, hs))) return rc;
    }
    if (fields_written) *fields_written = fields_written_word(shared != 0, want_c, want_f, false);
    return MI_OK;
}

}  // namespace mi

using namespace mi;

extern "C" {

int64_t mi_render_occupancy_clip_extra_bytes(int64_t n) { return n <= 0 ? 0 : clip_bounds_bytes(n); }

int64_t mi_render_occupancy_extra_bytes(int64_t n, int n_coarse, int n_fine) {
    if (n <= 0 || n_coarse < 1 || n_fine < 0) return 0;
    return OccLists(false, n, n_coarse, n_fine).bytes();
}

int64_t mi_render_occupancy_train_extra_bytes(int64_t n, int n_coarse, int n_fine) {
    if (n <= 0 || n_coarse < 1 || n_fine < 0 || n > 0x7fffffffLL / ((int64_t)n_coarse + n_fine)) return 0;
    return OccLists(true, n, n_coarse, n_fine).bytes();
}

int64_t mi_render_occupancy_train_saved_bytes(int kind_coarse, int kind_fine, int64_t n, int n_coarse, int n_fine) {
    if (int rc = check_call("mi_render_occupancy_train_saved_bytes", "training", kind_coarse, kind_fine, n, n_coarse, n_fine)) return rc;
    return saved_bytes_of(kind_coarse, kind_fine, n, n_coarse, n_fine);
}

int64_t mi_render_occupancy_backward_workspace_bytes(int kind_coarse, int kind_fine, int shared, int64_t n, int n_coarse, int n_fine) {
    if (int rc = check_call("mi_render_occupancy_backward_workspace_bytes", "training", kind_coarse, kind_fine, n, n_coarse, n_fine)) return rc;
    if (n == 0) return 0;
    return OccBwdLayout(kind_coarse, kind_fine, shared != 0, n, n_coarse, n_fine).bytes();
}

// each of the four forwards fills OccArgs in its members' order: its own parameters, null for what it does not take
int mi_render_rays_occupancy(int kind_coarse, const float* packed_coarse, int kind_fine, const float* packed_fine,
                             const float* rays, int64_t n, float near_, float far_, int n_coarse, int n_fine,
                             const float* z_lin, const float* u_lin, const float* t_rand, uint64_t seed, uint64_t ray0,
                             const uint32_t* bits, const int* dims, const float* lo, const float* inv_cell, float* rgb_c,
                             float* depth_c, float* acc_c, float* rgb_f, float* depth_f, float* acc_f, int* evaluated,
                             void* workspace, int64_t workspace_bytes, void* stream) {
    return occupancy_render("mi_render_rays_occupancy", OCC_RENDER, nullptr,
                            {kind_coarse, packed_coarse, kind_fine, packed_fine, rays, n, near_, far_, n_coarse, n_fine, z_lin, u_lin,
                             t_rand, seed, ray0, bits, dims, lo, inv_cell, rgb_c, depth_c, acc_c, rgb_f, depth_f, acc_f, evaluated,
                             workspace, workspace_bytes, nullptr, 0, stream});
}

int mi_render_rays_occupancy_clip(int kind_coarse, const float* packed_coarse, int kind_fine, const float* packed_fine,
                                  const float* rays, int64_t n, float near_, float far_, int n_coarse, int n_fine, int probes,
                                  int pad, const float* u_lin, const float* t_rand, uint64_t seed, uint64_t ray0,
                                  const uint32_t* bits, const int* dims, const float* lo, const float* inv_cell, float* rgb_c,
                                  float* depth_c, float* acc_c, float* rgb_f, float* depth_f, float* acc_f, int* evaluated,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
    OccClip clip{probes, pad, nullptr};
    return occupancy_render("mi_render_rays_occupancy_clip", OCC_RENDER, &clip,
                            {kind_coarse, packed_coarse, kind_fine, packed_fine, rays, n, near_, far_, n_coarse, n_fine, nullptr, u_lin,
                             t_rand, seed, ray0, bits, dims, lo, inv_cell, rgb_c, depth_c, acc_c, rgb_f, depth_f, acc_f, evaluated,
                             workspace, workspace_bytes, nullptr, 0, stream});
}

int mi_render_rays_occupancy_train(int kind_coarse, const float* packed_coarse, int kind_fine, const float* packed_fine,
                                   const float* rays, int64_t n, float near_, float far_, int n_coarse, int n_fine,
                                   const float* z_lin, const float* u_lin, const float* t_rand, uint64_t seed, uint64_t ray0,
                                   const uint32_t* bits, const int* dims, const float* lo, const float* inv_cell, float* rgb_c,
                                   float* depth_c, float* acc_c, float* rgb_f, float* depth_f, float* acc_f, int* evaluated,
                                   void* workspace, int64_t workspace_bytes, void* saved, int64_t saved_bytes, void* stream) {
    return occupancy_render("mi_render_rays_occupancy_train", OCC_TRAIN, nullptr,
                            {kind_coarse, packed_coarse, kind_fine, packed_fine, rays, n, near_, far_, n_coarse, n_fine, z_lin, u_lin,
                             t_rand, seed, ray0, bits, dims, lo, inv_cell, rgb_c, depth_c, acc_c, rgb_f, depth_f, acc_f, evaluated,
                             workspace, workspace_bytes, saved, saved_bytes, stream});
}

int mi_render_rays_occupancy_clip_train(int kind_coarse, const float* packed_coarse, int kind_fine, const float* packed_fine,
                                        const float* rays, int64_t n, float near_, float far_, int n_coarse, int n_fine, int probes,
                                        int pad, const float* u_lin, const float* t_rand, uint64_t seed, uint64_t ray0,
                                        const uint32_t* bits, const int* dims, const float* lo, const float* inv_cell, float* rgb_c,
                                        float* depth_c, float* acc_c, float* rgb_f, float* depth_f, float* acc_f, int* evaluated,
                                        void* workspace, int64_t workspace_bytes, void* saved, int64_t saved_bytes, void* stream) {
    OccClip clip{probes, pad, nullptr};
    return occupancy_render("mi_render_rays_occupancy_clip_train", OCC_TRAIN, &clip,
                            {kind_coarse, packed_coarse, kind_fine, packed_fine, rays, n, near_, far_, n_coarse, n_fine, nullptr, u_lin,
                             t_rand, seed, ray0, bits, dims, lo, inv_cell, rgb_c, depth_c, acc_c, rgb_f, depth_f, acc_f, evaluated,
                             workspace, workspace_bytes, saved, saved_bytes, stream});
}

int mi_render_rays_occupancy_backward(int kind_coarse, const float* packed_bwd_coarse, int kind_fine,
                                      const float* packed_bwd_fine, int shared, const float* rays, int64_t n, int n_coarse,
                                      int n_fine, const void* workspace, int64_t workspace_bytes, const void* saved,
                                      int64_t saved_bytes, const float* g_rgb_c, const float* g_depth_c, const float* g_acc_c,
                                      const float* g_rgb_f, const float* g_depth_f, const float* g_acc_f,
                                      float* const* grad_params_coarse, float* const* grad_params_fine, void* bwd_workspace,
                                      int64_t bwd_workspace_bytes, int* fields_written, void* stream) {
    return occupancy_backward("mi_render_rays_occupancy_backward", kind_coarse, packed_bwd_coarse, kind_fine, packed_bwd_fine, shared, rays, n,
                              n_coarse, n_fine, workspace, workspace_bytes, saved, saved_bytes, g_rgb_c, g_depth_c, g_acc_c, g_rgb_f,
                              g_depth_f, g_acc_f, grad_params_coarse, grad_params_fine, bwd_workspace, bwd_workspace_bytes, fields_written,
                              nullptr, 0, nullptr, 0, nullptr, stream);
}

int mi_render_rays_occupancy_backward_rays(int kind_coarse, const float* packed_bwd_coarse, int kind_fine,
                                           const float* packed_bwd_fine, int shared, const float* rays, int64_t n, int n_coarse,
                                           int n_fine, const void* workspace, int64_t workspace_bytes, const void* saved,
                                           int64_t saved_bytes, const float* g_rgb_c, const float* g_depth_c, const float* g_acc_c,
                                           const float* g_rgb_f, const float* g_depth_f, const float* g_acc_f,
                                           float* const* grad_params_coarse, float* const* grad_params_fine, void* bwd_workspace,
                                           int64_t bwd_workspace_bytes, int* fields_written, const float* const* params_coarse,
                                           int n_params_coarse, const float* const* params_fine, int n_params_fine, float* g_rays,
                                           void* stream) {
    const char* fn = "mi_render_rays_occupancy_backward_rays";
    if (!g_rays) { if (fields_written) *fields_written = 0; set_error("%s: null pointer argument (g_rays)", fn); return MI_EINVAL; }
    return occupancy_backward(fn, kind_coarse, packed_bwd_coarse, kind_fine, packed_bwd_fine, shared, rays, n, n_coarse, n_fine, workspace,
                              workspace_bytes, saved, saved_bytes, g_rgb_c, g_depth_c, g_acc_c, g_rgb_f, g_depth_f, g_acc_f,
                              grad_params_coarse, grad_params_fine, bwd_workspace, bwd_workspace_bytes, fields_written, params_coarse,
                              n_params_coarse, params_fine, n_params_fine, g_rays, stream);
}

}  // extern "C"
