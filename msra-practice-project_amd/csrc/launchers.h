// launchers.h - the host launchers of every kernel unit of libmirender (gfx950 only) and their size queries, with the
// occupancy-grid argument structs and the stop constants that are their contracts.  The units that call them are the cheap
// host units; each unit that defines one includes this, so a changed signature is caught where it is defined.  The four MFMA
// kernel units do not: the chain's launcher pair is in field_bwd.h, the forward's launchers in field_mlp.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mi_device.h"

namespace mi {

// host launchers (field_mlp.hip, field_bwd_dw.hip, render_stages.hip, eval_stages.hip, adam_step.hip)
// sigma_only: the kind's sigma-only instance (has_sigma_only_kernel), which writes sigma alone to a.out [M]
int launch_mlp(int kind, const MlpArgs& a, int64_t n_groups, hipStream_t stream, bool sigma_only = false);
bool has_sigma_only_kernel(int kind);
// the sigma-only instance over a window of samples of the live rays (a.live_rays / a.live_count / a.n_rays / a.win_*;
// a.a = rays, a.z and a.out [n_rays, n_samples]); the grid covers n_rays, blocks past the live count return at once
int launch_mlp_window(int kind, const MlpArgs& a, hipStream_t stream);
// The fine pass with its colour branch deferred to the points with sigma > 0 (NeRF, TinyNeRF: has_deferred_colour_kernels).
// launch_mlp_trunk_spill: a mode-1 launch of one group that writes {0, 0, 0, sigma} to a.out [points][4] and appends every
// point with sigma > 0 to the list d; launch_mlp_colour: the colour branch over that list, r, g, b into a.out (same a).
bool has_deferred_colour_kernels(int kind);
int launch_mlp_trunk_spill(int kind, const MlpArgs& a, const DeferArgs& d, hipStream_t stream);
int launch_mlp_colour(int kind, const MlpArgs& a, const DeferArgs& d, hipStream_t stream);
// occupancy.hip: construction of a per-scene occupancy bit grid (include/mi_render.h)
int launch_occupancy_cell_points(const int* dims, const float* lo, const float* cell, int k, int64_t head, int64_t count,
                                 float* points, hipStream_t stream);
int64_t occupancy_pack_workspace_bytes(int64_t cells, int dilate);
int launch_occupancy_pack(const float* sigma, const int* dims, int k, float threshold, int dilate, uint32_t* bits,
                          void* workspace, hipStream_t stream);
// ... a live grid's density (mi_occupancy_draw_points / _density_update / _density_pack): the rows' cells and jittered points,
// the fold of their sigma into density (the first region of the workspace: the scratch ints) and the re-thresholding into bits
int launch_occupancy_draw_points(const uint32_t* bits, const int* dims, const float* lo, const float* cell, uint64_t seed,
                                 uint32_t epoch, int mode, int64_t row0, int64_t count, int64_t n_uniform, int* cell_ids,
                                 float* points, hipStream_t stream);
int64_t occupancy_density_workspace_bytes(int64_t cells, int dilate);
int launch_occupancy_density_update(const float* sigma, const int* cell_ids, int64_t count, const int* dims, float decay,
                                    float* density, void* workspace, hipStream_t stream);
int launch_occupancy_density_pack(const float* density, const int* dims, float threshold, int relative, int dilate, uint32_t* bits,
                                  void* workspace, hipStream_t stream);
// ... and reading one.  A grid as the kernels take it: box and cells by value (MarkArgs, a kernel argument) and the device words.
// occupancy_grid_args (render_path.h) is the one place a caller's grid is checked and copied into one.
struct MarkArgs { int dims[3]; float lo[3], inv_cell[3]; };
struct OccupancyGridArgs { MarkArgs cells; const uint32_t* bits; };
// The samples of n rays x S depths that lie in occupied cells, appended to `list` (point indices ray * S + k,
// any order) and counted in the device int `count`, which the call clears; the raw rows [n*S][4] of the others are zeroed
// (raw may be null).  n * S fits an int (the caller checks).
int launch_occupancy_mark_rays(const OccupancyGridArgs& grid, const float* rays, const float* z, int64_t n, int S, int* list,
                               int* count, float* raw, hipStream_t stream);
// ... and the same list in ASCENDING order, written without atomics (a count per workgroup, a scan, a scatter): the order a
// training step needs, whose weight-gradient sums run over the list's rows.  `list` has room for
// occupancy_ordered_list_ints(n * S) ints: the entries, then one scan slot per workgroup.
int64_t occupancy_ordered_list_ints(int64_t points);
int launch_occupancy_mark_rays_ordered(const OccupancyGridArgs& grid, const float* rays, const float* z, int64_t n, int S, int* list,
                                       int* count, float* raw, hipStream_t stream);
// Each ray's sampling range clipped to the grid (the rule: occupancy.hip, include/mi_render.h): bounds [n,2] = (near_r, far_r),
// (near_, far_) for a ray none of whose `probes` probes is occupied.  1 <= probes <= 4096, pad >= 0, near_ < far_ (the caller checks).
int launch_occupancy_clip_rays(const OccupancyGridArgs& grid, const float* rays, int64_t n, float near_, float far_, int probes,
                               int pad, float* bounds, hipStream_t stream);
// The inference forward over a device-counted list of point indices (NeRF, SirenNeRF, TinyNeRF: has_list_kernel): a mode-1
// launch of one group (a.a = rays, a.z and a.out [rays_per_group * n_samples]) that evaluates point list[e] for every e below
// *count and writes its row a.out[list[e]] alone.  The grid covers every point of the launch (host values, no read-back);
// blocks past the count return at once.  With a.save set it is the training forward over the list (the FWD_LIST_SAVE
// instances): the saved rows of entry e are written at row e of every region (compact; a.save_points = the capacity, the
// regions' stride), rows at and past the count are not written.
bool has_list_kernel(int kind);
int launch_mlp_list(int kind, const MlpArgs& a, const int* list, const int* count, hipStream_t stream);
// Backward of a field over the first *count rows of compact acts (launch_mlp_list with a.save): the chain reads raw / g_raw at
// rows list[e], writes dA rows e; the weight-gradient kernels contract rows [0, *count) in n_slabs slabs planned from the
// capacity, each counted_slab_pts(*count, n_slabs) long.  Non-FiLM kinds.  No host read-back.
int launch_field_backward_list(int kind, const float* packed_bwd, const float* acts, float* grads, const float* raw,
                               const float* g_raw, const int* list, const int* count, int64_t capacity, float* partial,
                               float* const* gp, hipStream_t stream);
int64_t bwd_partial_floats(int64_t P);
int64_t film_partial_floats(int64_t n_groups, int64_t points_per_group);
int64_t bwd_partial_floats_kind(int kind, int64_t P);                      // ... of any kind (deeper FiLM kinds need more)
int64_t film_partial_floats_kind(int kind, int64_t n_groups, int64_t points_per_group);
int launch_field_backward(int kind, const float* packed_bwd, const float* acts, float* grads, const float* raw,
                          const float* g_raw, int64_t n_groups, int64_t points_per_group, const float* film,
                          float* film_partial, float* grad_film, float* partial, float* const* gp,
                          const float* const* params, hipStream_t stream);
int launch_gen_rays(int width, int height, double focal, const float* c2w, int64_t ray0, int64_t n, float* rays,
                    int compute_f64, hipStream_t stream);
int launch_sample_coarse(int64_t n, float near_, float far_, int nc, const float* z_lin, const float* t_rand,
                         uint64_t seed, uint64_t ray0, float* z, hipStream_t stream);
int launch_composite(int64_t n, int S, const float* raw, const float* z, const float* rays, float* rgb, float* depth,
                     float* acc, float* weights, hipStream_t stream);
int launch_composite_weights(int64_t n, int S, const float* sigma, int sigma_stride, const float* z, const float* rays,
                             float* depth, float* acc, float* weights, hipStream_t stream);
// The epsilon sample_pdf adds to every weight before it normalises them (render.py:31); normalise_pdf (render_stages.hip)
// is its one user.
constexpr float kPdfEps = 1e-5f;
// ulp of a positive normal float: 2^-23 times the power of two at or below it
constexpr double float_ulp(float x) {
    double p = 1.0;
    while (p > (double)x) p *= 0.5;
    while (p * 2.0 <= (double)x) p *= 2.0;
    return p * 0x1p-23;
}
// Where the resumable weights composite stops a ray: at a window boundary whose fp64 running product D is <= the threshold.
//   * kStopZeroWeight, 2^-151: every later weight is exactly 0.0f (composite_weights_window_kernel's comment), so every
//     consumer of the weights, the sums depth_c / acc_c included, keeps its bits.
//   * kStopBelowPdfEps, 2^-42, for a coarse pass whose only product is the weights that sample_fine reads.  normalise_pdf
//     uses a weight only as w + kPdfEps, in the sum and in the quotient, un-fused (-ffp-contract=off).  kPdfEps lies in
//     [2^-17, 2^-16), so its ulp is 2^-40 and every 0 <= w < 2^-41, half an ulp, gives fl(w + kPdfEps) == kPdfEps whichever
//     way a tie would round: such a weight is indistinguishable from 0.  A later sample's weight is
//     alpha * (float)(T * excl) with alpha in [0, 1] and the factors f = (1-alpha)+1e-10f <= 1 (sigma >= 0, ascending
//     depths), so the exact product can only fall: no later weight exceeds the transmittance in front of it, whatever its
//     sigma is.  The scans' products differ from the exact ones by a relative 2^-45 at most, and rounding to float adds
//     2^-24: far inside the factor 2 between the threshold, a quarter ulp, and the half ulp - the margin 2^-151 keeps under
//     2^-150.  Zero weights behind the stop therefore give the same pdf, cdf, z_samples and z_fine bits, and the fine
//     outputs keep theirs.  depth_c and acc_c add every weight, however small: a call that asks for either keeps 2^-151.
constexpr double kStopZeroWeight = 0x1p-151;
constexpr double kStopBelowPdfEps = 0x1p-42;
static_assert(kStopBelowPdfEps <= 0.25 * float_ulp(kPdfEps),
              "a weight below half an ulp of kPdfEps vanishes in w + kPdfEps; the stop keeps a factor 2 under that");
static_assert(kStopZeroWeight <= kStopBelowPdfEps, "the early stop never waits longer than the exact one");

// composite_weights over samples [0, k1) of the live rays, k1 > k0 the end of the window just evaluated: writes the weights
// of [k0, k1), appends the rays that can still contribute behind k1 to live_out, finishes the others (zero weights behind
// k1, depth / acc); live_out null = the last window, every ray is finished.  stop: kStopZeroWeight or kStopBelowPdfEps
int launch_composite_weights_window(int64_t n, int S, const float* sigma, const float* z, const float* rays, float* depth,
                                    float* acc, float* weights, const int* live_in, const int* count_in, int* live_out,
                                    int* count_out, int k0, int k1, double stop, hipStream_t stream);
int launch_composite_bwd(int64_t n, int S, const float* raw, const float* z, const float* rays, const float* g_rgb,
                         const float* g_depth, const float* g_acc, const float* g_w, float* g_raw, hipStream_t stream);
int launch_composite_bwd_rays(int64_t n, int S, const float* raw, const float* z, const float* rays, const float* g_rgb,
                              const float* g_depth, const float* g_acc, const float* g_w, int accumulate, float* g_rays,
                              hipStream_t stream);
// ray_grad.hip: dL/d(field inputs) of the points of one launch_field_backward call, from the acts / grads it left behind
int launch_field_input_grad(int kind, const float* const* params, const float* film, const float* acts, const float* grads,
                            int64_t n_groups, int64_t points_per_group, float* g_x, hipStream_t stream);
int launch_field_input_grad_rays(int kind, const float* const* params, const float* film, const float* acts,
                                 const float* grads, const float* rays, const float* z, int64_t n_groups,
                                 int64_t rays_per_group, int n_samples, int accumulate, float* g_rays, hipStream_t stream);
// ... of the rays of one launch_field_backward_list call (non-FiLM kinds), from the COMPACT acts / grads rows it left behind:
// ray r's samples are the run of the ascending list inside [r S, (r + 1) S), found on the device; entry e reads row e of every
// region (stride: the capacity n * n_samples, which fits an int) and z[list[e]].  Sized from n; no read-back, no atomics.
int launch_field_input_grad_rays_list(int kind, const float* const* params, const float* acts, const float* grads,
                                      const int* list, const int* count, const float* rays, const float* z, int64_t n,
                                      int n_samples, int accumulate, float* g_rays, hipStream_t stream);
int64_t image_metrics_workspace_floats(int images, int channels, int H, int W);
int launch_image_metrics(const float* img1, const float* img2, int images, int channels, int H, int W,
                         const float* window, int window_size, float* workspace, float* out, hipStream_t stream);
int launch_grid_points(int N, const float* origin, float voxel_size, int64_t head, int64_t count, float* pts,
                       hipStream_t stream);
int64_t nerf_loss_workspace_floats(int64_t n);
int launch_nerf_loss(int64_t n, const float* rgb_c, const float* acc_c, const float* rgb_f, const float* acc_f,
                     const float* target, int use_alpha, int use_fine, float* g_rgb_c, float* g_acc_c, float* g_rgb_f,
                     float* g_acc_f, float* workspace, float* out, hipStream_t stream);
int launch_ray_bank(int width, int height, double focal, const float* poses, const float* rgba, int white_bkgd,
                    int64_t images, float* out, int compute_f64, hipStream_t stream);
int launch_pack(int kind, StreamDir dir, const float* const* params, int n_params, float w0, float* packed,
                hipStream_t stream);
int launch_adam_step(int n_fields, const int* kinds, const int* n_params, float* const* params, const float* const* grads,
                     float* const* exp_avg, float* const* exp_avg_sq, const int64_t* numel, float step_size,
                     float one_minus_beta1, float beta2, float one_minus_beta2, float eps, float bc2_sqrt,
                     float* const* packed_fwd, float* const* packed_bwd, hipStream_t stream);
int launch_sample_pdf(int64_t n, int nb, int ns, const float* bins, const float* weights, const float* u_lin, float* out,
                      hipStream_t stream);
int launch_sample_fine(int64_t n, float near_, float far_, int nc, int nf, const float* z_lin, const float* u_lin,
                       const float* z_coarse, const float* weights, float* z_samples, float* z_fine, int* pos,
                       hipStream_t stream);
// ... and both samplers over a range per ray, bounds [n,2] = (near_r, far_r): the same arithmetic, the coarse linspace evaluated in
// the kernel from the ray's own two floats (no z_lin table)
int launch_sample_coarse_bounds(int64_t n, const float* bounds, int nc, const float* t_rand, uint64_t seed, uint64_t ray0,
                                float* z, hipStream_t stream);
int launch_sample_fine_bounds(int64_t n, const float* bounds, int nc, int nf, const float* u_lin, const float* z_coarse,
                              const float* weights, float* z_samples, float* z_fine, int* pos, hipStream_t stream);
int launch_merge_raw(int64_t n, int nc, int nf, const float* raw_c, const float* raw_s, const int* pos, float* raw_f,
                     hipStream_t stream);
int launch_split_grad(int64_t n, int nc, int nf, const float* g_f, const int* pos, float* g_c, int accumulate_coarse,
                      float* g_s, hipStream_t stream);
// out[0, count) = 0.f (zero bits: an int buffer's clear too), by a kernel: a captured hipMemsetAsync does not replay reliably
int launch_clear_floats(int64_t count, float* out, hipStream_t stream);

}  // namespace mi
