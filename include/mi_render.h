/*
 * mi_render.h - C ABI of libmirender.so: the MI355X (gfx950) implementation of the
 * ray-march -> field-MLP -> alpha-composite path of JeffreyXiang/MSRA-practice-project.
 *
 * The reference has NO plugin/FFI layer: its boundary is the Python
 * module namespace `render` (nerf/render.py, pi_GAN/render.py).  Each entry point below
 * therefore cites the reference *Python function* whose device work it replaces; the
 * Python drop-in modules (msra-practice-project_amd/nerf/render.py, .../pi_GAN/render.py)
 * keep the reference call surface and bind these symbols with ctypes.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous fp32 unless stated otherwise;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - no allocation, no synchronisation inside: callers pass outputs and workspace;
 *   - return 0 on success, negative MI_E* on error; mi_last_error() gives the message
 *     (thread-local);
 *   - all launches are asynchronous on `stream`.
 */
#ifndef MI_RENDER_H
#define MI_RENDER_H

#include <stdint.h>

#include "mi_render_kinds.h"   /* the status codes MI_OK / MI_E* and the field-kind ids MI_FIELD_* */

#ifdef __cplusplus
extern "C" {
#endif

/* Library / build identification. */
int mi_abi_version(void);
const char* mi_last_error(void);

/* ---- field weights -------------------------------------------------------------- */

/* Number of (weight, bias) tensors the kind's state dict holds, in forward order
 * (weight_0, bias_0, weight_1, bias_1, ...). */
int mi_field_num_params(int kind);
/* Floats in the packed MFMA-ordered weight stream of the kind. */
int64_t mi_field_packed_floats(int kind);
/* Multiply-accumulates of the kind's linear layers per point (roofline accounting). */
int64_t mi_field_macs(int kind);
/* Rows of the kind's FiLM table (one gamma|beta row of 512 per FiLM layer): 9 for kinds 2 and 3, hidden_layers + 1 for
 * MI_FIELD_FILM_DEPTH kinds, 0 for the kinds without FiLM. */
int mi_field_film_layers(int kind);
/* Shape of parameter tensor `index` (0 <= index < mi_field_num_params(kind)): weights [rows = out, cols = in], biases
 * [rows = out, cols = 1].  What a host that does not hold an nn.Module needs in order to lay out the tensors it hands to
 * mi_field_pack (the shapes of nerf/nerf.py:59-73, 128-146 and pi_GAN/modules.py:76-94). */
int mi_field_param_shape(int kind, int index, int64_t* rows, int64_t* cols);
/* Repack torch-layout parameters ([out,in] row-major weights, [out] biases; `params` is a
 * HOST array of n_params device pointers in state-dict order) into the packed stream the
 * fused MLP kernel consumes.  Replaces nothing in the reference: it is the hand-off from
 * nn.Module parameters (nerf/nerf.py:59-73, pi_GAN/modules.py:76-94) to the kernel and is
 * called whenever the optimiser has changed the weights.
 * w_0: the frequency of the kind's sin layers, sin(w_0 (gamma (W x + b) + beta)) - FilmSiren's constructor argument
 * (pi_GAN/modules.py:11,22-25,73), any finite w_0 > 0, for the two FiLM kinds; every other kind has no such parameter
 * (Siren hard-codes 30, nerf/nerf.py:112) and takes 30 only.  It travels in the stream (a trailer piece the kernels read as a
 * wave-uniform scalar), so every entry point that consumes the stream evaluates the field it was packed for. */
int mi_field_pack(int kind, const float* const* params, int n_params, float w_0, float* packed, void* stream);

/* ---- fused field MLP forward ---------------------------------------------------- */

/* network(inputs[M,6]) -> [M,4] = (r,g,b,sigma): replaces the model call inside
 * run_network (nerf/render.py:72-74) for a known kind.
 *   x      [n_groups*points_per_group, 6]  (xyz, view_dir)
 *   film   [n_groups, mi_field_film_layers(kind), 512] FiLM table (gamma|beta per layer;
 *          pi_GAN/modules.py:96-99) for FILM kinds, else NULL; group g uses film[g]
 *   out    [n_groups*points_per_group, 4] */
int mi_field_eval_points(int kind, const float* packed, const float* film, const float* x,
                         int64_t n_groups, int64_t points_per_group, float* out, void* stream);

/* run_network fused with point generation (nerf/render.py:134-135 / :143-144):
 * pts = o + d*z, view = d/|d|, raw = network([pts, view]).
 *   rays   [n_groups*rays_per_group, 2, 3] (origin, direction)
 *   z      [n_groups*rays_per_group, S]
 *   raw    [n_groups*rays_per_group, S, 4] */
int mi_field_eval_rays(int kind, const float* packed, const float* film, const float* rays,
                       const float* z, int64_t n_groups, int64_t rays_per_group, int n_samples,
                       float* raw, void* stream);

/* ---- sampling / compositing stages ---------------------------------------------- */

/* get_rays (nerf/render.py:7-23) on device, written in render_image's ray-list order
 * (render.py:151-154): rays[ray0 .. ray0+n) of the H*W list, c2w = 12 floats (3x4 row-major,
 * HOST pointer).  compute_f64 = 0 reproduces NumPy with a Python-float focal (all fp32);
 * compute_f64 = 1 reproduces an np.float64 focal (pi_GAN/modules.py:127: fp64 math, rounded to
 * fp32 at the end).  out rays [n,2,3]. */
int mi_gen_rays(int width, int height, double focal, const float* c2w_host, int64_t ray0, int64_t n,
                float* rays, int compute_f64, void* stream);

/* stratified depths (nerf/render.py:123-132): z = lower + (upper-lower)*t_rand.
 * z_lin  [Nc] optional table = linspace(near,far,Nc) (pass torch.linspace's CPU output for
 *        bit parity with the CPU reference; NULL = ATen's scalar formula computed in-kernel)
 * t_rand [n,Nc] device pointer, or NULL to draw U[0,1) from Philox4x32-10 keyed by
 *        (seed, ray0 + ray index, sample index): ray0 = the index of this call's first ray in the
 *        caller's larger ray list, so a frame's jitter does not depend on how it is split over calls
 *        or GPUs.  out z [n,Nc]. */
int mi_sample_coarse(int64_t n, float near_, float far_, int n_coarse, const float* z_lin,
                     const float* t_rand, uint64_t seed, uint64_t ray0, float* z, void* stream);

/* raw_to_outputs (nerf/render.py:78-103).  raw [n,S,4], z [n,S], rays [n,2,3] (direction
 * used for |d|).  out rgb [n,3], depth [n], acc [n], weights [n,S] (weights may be NULL). */
int mi_composite(int64_t n, int n_samples, const float* raw, const float* z, const float* rays,
                 float* rgb, float* depth, float* acc, float* weights, void* stream);

/* sample_pdf + sort (nerf/render.py:140-142): bins = mids of linspace(near,far,Nc),
 * weights[...,1:-1] of the coarse pass, deterministic u = linspace(0,1,Nf), merged with
 * the coarse depths and sorted.  z_lin [Nc] / u_lin [Nf]: optional tables as above.
 * out z_fine [n,Nc+Nf]; z_samples [n,Nf] optional (NULL). */
int mi_sample_fine(int64_t n, float near_, float far_, int n_coarse, int n_fine, const float* z_lin,
                   const float* u_lin, const float* z_coarse, const float* weights, float* z_samples,
                   float* z_fine, void* stream);

/* The same, also returning where every input element went: pos [n, Nc+Nf] int32, pos[e] = index in z_fine of
 * z_coarse[e] (e < Nc) or of z_samples[e - Nc].  What a renderer needs to evaluate ONE field shared by both passes
 * (pi_GAN/modules.py:160-161 passes the same model twice; nerf/train_nerf.py:91,94 with use_fine_model off) at the Nf new
 * depths only: the fine pass of nerf/render.py:143-144 re-evaluates the Nc coarse points with the same field. */
int mi_sample_fine_pos(int64_t n, float near_, float far_, int n_coarse, int n_fine, const float* z_lin,
                       const float* u_lin, const float* z_coarse, const float* weights, float* z_samples,
                       float* z_fine, int* pos, void* stream);

/* raw_fine [n,Nc+Nf,4] in sorted order out of the coarse pass's raw_coarse [n,Nc,4] and raw_samples [n,Nf,4] (the field at
 * z_samples): raw_fine[pos[e]] = e < Nc ? raw_coarse[e] : raw_samples[e - Nc].  Replaces the second field call of
 * nerf/render.py:144 when both passes share one field; bit-identical to it. */
int mi_merge_raw(int64_t n, int n_coarse, int n_fine, const float* raw_coarse, const float* raw_samples, const int* pos,
                 float* raw_fine, void* stream);

/* The transpose of mi_merge_raw for the backward pass: g_raw_coarse[e] (+)= g_raw_fine[pos[e]] (+= when
 * accumulate_coarse: onto the coarse outputs' own gradient), g_raw_samples[i] = g_raw_fine[pos[Nc + i]]. */
int mi_split_grad(int64_t n, int n_coarse, int n_fine, const float* g_raw_fine, const int* pos, float* g_raw_coarse,
                  int accumulate_coarse, float* g_raw_samples, void* stream);

/* sample_pdf as a free-standing function (nerf/render.py:27-56; star-imported by the reference's scripts):
 * bins [n,n_bins], weights [n,n_bins-1] -> samples [n,n_samples]; u_lin [n_samples] optional table as above. */
int mi_sample_pdf(int64_t n, int n_bins, int n_samples, const float* bins, const float* weights,
                  const float* u_lin, float* samples, void* stream);

/* ---- whole path ----------------------------------------------------------------- */

/* render_rays (nerf/render.py:106-147) for known field kinds, all stages on `stream`.
 *   rays [n,2,3]; n = n_groups*rays_per_group; film tables as in mi_field_eval_rays
 *   outs: rgb_c[n,3] depth_c[n] acc_c[n] rgb_f[n,3] depth_f[n] acc_f[n]
 *   seed, ray0: as in mi_sample_coarse (used when t_rand is NULL)
 *   workspace: mi_render_workspace_bytes(n, Nc, Nf) bytes; workspace_bytes = what the caller really provided.
 *   When both passes share one field (same kind, same packed pointer) and the workspace also holds
 *   mi_render_shared_field_extra_bytes(n, Nc, Nf) more, the fine pass evaluates the Nf new depths only (mi_merge_raw);
 *   with Nf = 0 it aliases the coarse outputs.  Results are bit-identical either way.
 *   The coarse outputs are optional: rgb_c = NULL says the coarse colours are not wanted, and then depth_c and acc_c may
 *   each be NULL too (with rgb_c, all three are needed).  The fine outputs, rays and the workspace are not optional.
 *   Without rgb_c and with two different fields (kind or packed pointer), the coarse pass runs the coarse field's
 *   sigma-only forward, where the kind has one (NeRF, SirenNeRF, TinyNeRF), and a composite that forms the weights (and
 *   depth_c / acc_c when asked for) from sigma alone.  The fine outputs, and depth_c / acc_c, are the same bits as those
 *   of a call with all six outputs.  That coarse pass runs front to back in windows of samples and stops evaluating the
 *   field along a ray once the ray's transmittance has reached zero: every later weight is exactly 0 whatever the field
 *   returns there, so no output bit depends on it - except that a non-finite sigma behind a zero transmittance no longer
 *   reaches the outputs as NaN.  All launches stay asynchronous, with host-known grid sizes (stream capture works).
 *   When depth_c and acc_c are NULL as well, the coarse weights have one reader left, the fine sampler, which uses a
 *   weight only as w + 1e-5f: that pass then stops along a ray as soon as the transmittance in front of a window is
 *   <= 2^-42.  No later weight can exceed the transmittance in front of it (alpha <= 1, and the running product only
 *   falls), and a weight below 2^-41, half an ulp of 1e-5f, leaves that sum unchanged: the fine depths and the fine
 *   outputs are still the same bits (64 + 128 samples, 800x800, one MI355X: the coarse launches take 42.8 instead of
 *   111.6 ms per frame, the frame 897.5 instead of 965.1 ms).  The caveat above then holds from that earlier point on:
 *   a non-finite sigma behind it no longer reaches the pixel.
 *   With two different fields, a fine field of a kind that has the kernels (NeRF, TinyNeRF), Nf > 0 and a workspace that
 *   also holds mi_render_deferred_colour_extra_bytes(n, Nc, Nf) more, the fine pass runs its colour branch only on the
 *   points with sigma > 0 (in chunks of whole rays: the trunk for every point, then the colour branch over the chunk's
 *   live points).  A point with sigma == 0 has weight exactly 0, so no output bit depends on its colour - except that a
 *   non-finite colour at such a point no longer reaches the outputs as NaN.  Without the extra bytes: the whole forward,
 *   same results. */
int64_t mi_render_workspace_bytes(int64_t n, int n_coarse, int n_fine);
int64_t mi_render_shared_field_extra_bytes(int64_t n, int n_coarse, int n_fine);
int64_t mi_render_deferred_colour_extra_bytes(int64_t n, int n_coarse, int n_fine);    /* 0 with Nf = 0 */
int mi_field_has_deferred_colour(int kind);    /* 1 if a fine field of this kind can use those bytes, else 0 (needs no GPU) */
int mi_render_rays(int kind_coarse, const float* packed_coarse, int kind_fine, const float* packed_fine,
                   const float* film, const float* rays, int64_t n_groups, int64_t rays_per_group,
                   float near_, float far_, int n_coarse, int n_fine, const float* z_lin, const float* u_lin,
                   const float* t_rand, uint64_t seed, uint64_t ray0, float* rgb_c, float* depth_c, float* acc_c,
                   float* rgb_f, float* depth_f, float* acc_f, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- training: what autograd does for the reference (train_nerf.py:151-168) ------------------ */

/* Backward of raw_to_outputs (nerf/render.py:91-103): dL/d(rgb, depth, acc, weights) -> dL/d(raw) [n,S,4].
 * Any of g_rgb [n,3], g_depth [n], g_acc [n], g_weights [n,S] may be NULL (= zero); g_weights is the cotangent of the
 * weights the function also returns (render.py:103; render_rays itself detaches what it derives from them, :141).
 * z and rays carry no gradient (z_samples is detached at render.py:141). */
int mi_composite_bwd(int64_t n, int n_samples, const float* raw, const float* z, const float* rays,
                     const float* g_rgb, const float* g_depth, const float* g_acc, const float* g_weights, float* g_raw,
                     void* stream);

/* Transposed weight stream for the backward chain (second packed buffer, refreshed with the weights). */
int64_t mi_field_packed_bwd_floats(int kind);
int mi_field_pack_bwd(int kind, const float* const* params, int n_params, float w_0, float* packed_bwd, void* stream);

/* Per-point sizes (floats) of the training buffers, or -1 if the kind has no backward yet:
 * acts = layer inputs saved by the training forward; grads = per-layer dA written by the backward chain.
 * mi_field_bwd_partial_floats(points) = scratch for the dW slab partial sums of the fixed kinds;
 * mi_field_bwd_partial_floats_kind(kind, points) = the same for any kind (MI_FIELD_FILM_DEPTH kinds deeper than 8 need more). */
int64_t mi_field_train_acts_floats(int kind);
int64_t mi_field_train_grads_floats(int kind);
int64_t mi_field_bwd_partial_floats(int64_t points);
int64_t mi_field_bwd_partial_floats_kind(int kind, int64_t points);

/* mi_field_eval_rays that also saves every linear layer's input into `acts`
 * [mi_field_train_acts_floats(kind) * points] (points = n_groups*rays_per_group*n_samples). */
int mi_field_eval_rays_train(int kind, const float* packed, const float* film, const float* rays, const float* z,
                             int64_t n_groups, int64_t rays_per_group, int n_samples, float* raw, float* acts,
                             void* stream);

/* mi_field_eval_points that also saves every linear layer's input (the training forward of `network(x)` called on
 * its own, nerf/render.py:73 outside render_rays): acts [mi_field_train_acts_floats(kind) * n_groups*points_per_group]. */
int mi_field_eval_points_train(int kind, const float* packed, const float* film, const float* x, int64_t n_groups,
                               int64_t points_per_group, float* out, float* acts, void* stream);

/* Backward of network(inputs) over n_groups*points_per_group points: g_raw [points,4] = dL/d(raw) ->
 * parameter gradients (and, for FiLM kinds, the gradient of the FiLM table).
 *   film            [n_groups,mi_field_film_layers(kind),512] FiLM table of the forward (FiLM kinds) or NULL
 *   grad_params     HOST array of n_params device pointers (torch layouts, state-dict order), OVERWRITTEN
 *   params          HOST array of the n_params parameter tensors themselves (FiLM kinds: the FiLM-table
 *                   gradient is formed from the per-image weight-gradient sums, d gamma = <W, dW_image> +
 *                   b . db_image); NULL for the other kinds
 *   grad_film       [n_groups,mi_field_film_layers(kind),512] (FiLM kinds) or NULL, OVERWRITTEN
 *   grads_ws        [mi_field_train_grads_floats(kind) * points]
 *   partial_ws      [mi_field_bwd_partial_floats_kind(kind, points)]
 *   film_partial_ws [mi_field_film_partial_floats_kind(kind, n_groups, points_per_group)] FiLM scratch (FiLM kinds) or
 *                   NULL; mi_field_film_partial_floats(n_groups, points_per_group) is the value for kinds 2 and 3 */
int64_t mi_field_film_partial_floats(int64_t n_groups, int64_t points_per_group);
int64_t mi_field_film_partial_floats_kind(int kind, int64_t n_groups, int64_t points_per_group);
int mi_field_backward(int kind, const float* packed_bwd, const float* film, const float* acts, float* grads_ws,
                      const float* raw, const float* g_raw, int64_t n_groups, int64_t points_per_group,
                      float* partial_ws, float* film_partial_ws, float* const* grad_params,
                      const float* const* params, int n_params, float* grad_film, void* stream);

/* ---- gradients to the field's inputs and to the rays (ray_grad.hip): opt-in, used by mirender/pose.py --------------
 * The reference's renderer is plain torch, so `pts = o + d z`, `view = d / |d|` and `dists * |d|`
 * (nerf/render.py:93,122,134,143) carry a gradient back to `rays` - what camera pose refinement differentiates.  The
 * three calls below produce it from buffers the training calls above leave behind; nothing above changes its results.
 *
 * mi_field_input_grad: dL/d(x) [points,6] (position | view direction, nerf/render.py:72) of the points of ONE
 * mi_field_backward call, called after it with the same kind / film / acts / grads_ws / n_groups / points_per_group.
 * `params` = HOST array of the n_params parameter tensors (device pointers, state-dict order), every kind.  g_x is
 * OVERWRITTEN.  Kinds whose rgb branch takes no direction (use_dir = False) give exactly 0 in columns 3..5.
 *
 * mi_field_input_grad_rays: the same gradient for points on rays (mi_field_eval_rays_train's inputs), reduced along
 * each ray without materialising [points,6]:  g_o = sum_s g_pos,s ;
 * g_d = sum_s z_s g_pos,s + (I - v v^T) / |d| sum_s g_dir,s with v = d / |d| (render.py:122,134).
 * g_rays [n,2,3]; accumulate != 0 adds to what it holds (the coarse and the fine pass both contribute to a ray),
 * 0 overwrites.  One wave owns a ray and no atomics are used: results do not vary from run to run.
 *
 * mi_composite_bwd_rays: the part of raw_to_outputs' backward that mi_composite_bwd leaves out (same arguments):
 * dists = delta_z * |d| (render.py:91-93), so dL/d|d| = sum_s dL/dalpha_s sigma_s delta_z_s exp(-sigma_s delta_z_s |d|)
 * and g_d = dL/d|d| * d / |d|, the last interval's delta_z = 1e10 included (sigma = 0 there gives an exact 0).
 * accumulate = 0 writes all six floats of a ray (g_o = 0), otherwise g_d is added to.  n_samples <= 4096.
 * The depths get no gradient: the stratified ones do not depend on the rays, the resampled ones are detached
 * (render.py:141). */
int mi_field_input_grad(int kind, const float* const* params, int n_params, const float* film, const float* acts,
                        const float* grads_ws, int64_t n_groups, int64_t points_per_group, float* g_x, void* stream);
int mi_field_input_grad_rays(int kind, const float* const* params, int n_params, const float* film, const float* acts,
                             const float* grads_ws, const float* rays, const float* z, int64_t n_groups,
                             int64_t rays_per_group, int n_samples, int accumulate, float* g_rays, void* stream);
int mi_composite_bwd_rays(int64_t n, int n_samples, const float* raw, const float* z, const float* rays,
                          const float* g_rgb, const float* g_depth, const float* g_acc, const float* g_weights,
                          int accumulate, float* g_rays, void* stream);

/* ---- training pair: render_rays forward + backward in two calls (train_path.hip) ----------------------------------
 * One iteration of nerf/train_nerf.py:151-168 from C (render_rays, the loss, loss.backward(), optimizer.step()), or the
 * generator backward of pi_GAN/modules.py:159-161: mi_render_rays_train -> mi_nerf_loss (or the caller's own loss) ->
 * mi_render_rays_backward -> mi_adam_step.  The pair restates what autograd does for render_rays in Python
 * (msra-practice-project_amd/mirender/autograd.py) and gives the same bits.
 *
 * Each pass (coarse: Nc samples per ray; fine: Nc + Nf with two fields, the Nf new depths with one shared field) is cut
 * into ray ranges of at most range_points points: whole rays; for FiLM kinds whole groups per range, or equal parts of
 * one group when one image alone is larger.  `saved` keeps the layer inputs of the leading ranges that fit in
 * saved_bytes (coarse pass first, each pass stopping at the first range that does not fit; any size, 0 included, gives
 * the same results); the backward re-runs the forward of every other range into its own workspace.
 *
 * mi_render_train_saved_bytes: what keeps every range (4 * mi_field_train_acts_floats * n * samples, summed over the
 * passes).  shared != 0: one field for both passes.
 * mi_render_backward_workspace_bytes: the backward's workspace for the given range split (n = n_groups*rays_per_group). */
int64_t mi_render_train_saved_bytes(int kind_coarse, int kind_fine, int shared, int64_t n, int n_coarse, int n_fine);
int64_t mi_render_backward_workspace_bytes(int kind_coarse, int kind_fine, int shared, int64_t n_groups,
                                           int64_t rays_per_group, int n_coarse, int n_fine, int64_t range_points_coarse,
                                           int64_t range_points_fine);

/* render_rays (nerf/render.py:106-147) with autograd's saved state: mi_render_rays' arguments and outputs, bit-identical
 * to it, plus the range split and the saved buffer.  The workspace (mi_render_workspace_bytes, and when both passes
 * share one field - same kind, same packed pointer - mi_render_shared_field_extra_bytes on top, else MI_EINVAL) holds
 * the forward's state afterwards: hand it to mi_render_rays_backward unchanged, with `saved`. */
int mi_render_rays_train(int kind_coarse, const float* packed_coarse, int kind_fine, const float* packed_fine,
                         const float* film, const float* rays, int64_t n_groups, int64_t rays_per_group, float near_,
                         float far_, int n_coarse, int n_fine, const float* z_lin, const float* u_lin, const float* t_rand,
                         uint64_t seed, uint64_t ray0, float* rgb_c, float* depth_c, float* acc_c, float* rgb_f,
                         float* depth_f, float* acc_f, void* workspace, int64_t workspace_bytes,
                         int64_t range_points_coarse, int64_t range_points_fine, void* saved, int64_t saved_bytes,
                         void* stream);

/* The backward of mi_render_rays_train (render_rays' part of loss.backward(), nerf/train_nerf.py:167): the six output
 * cotangents [n,3] / [n] (any may be NULL = no gradient) -> parameter gradients and the FiLM-table gradient.
 *   packed_* / packed_bwd_*: the fields' forward and transposed streams (mi_field_pack / mi_field_pack_bwd)
 *   params_*      HOST arrays of the parameter tensors (FiLM kinds; may be NULL for the others)
 *   film, rays, sizes, range points, workspace, saved: exactly as given to mi_render_rays_train (the depths come from
 *                 the workspace, so near / far and the linspace tables are not needed again)
 *   grad_params_* HOST arrays of mi_field_num_params device pointers, OVERWRITTEN.  A field that receives no cotangent
 *                 is left untouched and may pass NULL.  One shared field: both passes' sum goes to grad_params_coarse
 *                 (grad_params_fine is not used).
 *   grad_film     [n_groups,mi_field_film_layers(kind),512] (FiLM kinds), OVERWRITTEN with the sum of both passes' FiLM
 *                 gradients (two FiLM fields of one call share the table, so they have the same depth)
 *   bwd_workspace mi_render_backward_workspace_bytes
 *   fields_written HOST, optional: MI_WROTE_* bits of what was written; known from the NULL pattern, no synchronisation */
#define MI_WROTE_COARSE 1
#define MI_WROTE_FINE 2
#define MI_WROTE_FILM 4
int mi_render_rays_backward(int kind_coarse, const float* packed_coarse, const float* packed_bwd_coarse,
                            const float* const* params_coarse, int kind_fine, const float* packed_fine,
                            const float* packed_bwd_fine, const float* const* params_fine, const float* film,
                            const float* rays, int64_t n_groups, int64_t rays_per_group, int n_coarse, int n_fine,
                            int64_t range_points_coarse, int64_t range_points_fine, const void* workspace,
                            int64_t workspace_bytes, const void* saved, int64_t saved_bytes, const float* g_rgb_c,
                            const float* g_depth_c, const float* g_acc_c, const float* g_rgb_f, const float* g_depth_f,
                            const float* g_acc_f, float* const* grad_params_coarse, float* const* grad_params_fine,
                            float* grad_film, void* bwd_workspace, int64_t bwd_workspace_bytes, int* fields_written,
                            void* stream);

/* ---- evaluation stages (frame metrics, density grids) --------------------- */

/* Frame metrics of nerf/test_nerf.py:102-105: mean squared error (psnr = -10 log10 mse) and
 * pytorch_ssim.ssim (nerf/pytorch_ssim/__init__.py:12-37, 66-73: gaussian window, zero padding, groups =
 * channels, C1 = 0.01^2, C2 = 0.03^2) of two image batches [images][channels][height][width] (planar, as the
 * reference passes them: NCHW).  window: HOST array of window_size (odd, <= 31) normalised 1-D gaussian taps
 * (the reference's gaussian(window_size, 1.5), __init__.py:7-10); the 2-D window is its outer product.
 *   out [images][2] = {mse, mean ssim} per image (size_average=True is their mean: images have equal size)
 *   workspace [mi_image_metrics_workspace_floats(...)] */
int64_t mi_image_metrics_workspace_floats(int images, int channels, int height, int width);
int mi_image_metrics(const float* img1, const float* img2, int images, int channels, int height, int width,
                     const float* window, int window_size, float* workspace, float* out, void* stream);

/* Query points of create_mesh's voxel grid (pi_GAN/utils.py:57-75): for overall index i in [head, head+count):
 * (x,y,z) = (i/N/N%N, i/N%N, i%N) * voxel_size + (origin[2], origin[1], origin[0]) - the reference's axis
 * order - and a zero view direction.  voxel_origin: HOST array of 3 floats.  out points [count,6], ready for
 * mi_field_eval_points. */
int mi_grid_points(int n, const float* voxel_origin, float voxel_size, int64_t head, int64_t count, float* points,
                   void* stream);

/* ---- nerf training-loop data path ------------------------------------ */

/* nerf/train_nerf.py:158-167 in one pass over the batch: loss_x = mean((rgb_x - rgb)^2) [+ 0.1 mean((acc_x -
 * alpha)^2) if use_alpha]; loss = loss_fine [+ loss_coarse if use_fine_model].  target [n,4] = (r,g,b,alpha)
 * (batch[:, -4:]).  Writes the gradient seeds d loss / d(rgb_c [n,3], acc_c [n], rgb_f [n,3], acc_f [n]) that
 * render_rays' backward consumes, and out[4] = {loss, mean((rgb_fine - rgb)^2) (psnr = -10 log10 of it),
 * loss_coarse, loss_fine}.  workspace [mi_nerf_loss_workspace_floats(n)]. */
int64_t mi_nerf_loss_workspace_floats(int64_t n);
int mi_nerf_loss(int64_t n, const float* rgb_c, const float* acc_c, const float* rgb_f, const float* acc_f,
                 const float* target, int use_alpha, int use_fine_model, float* g_rgb_c, float* g_acc_c,
                 float* g_rgb_f, float* g_acc_f, float* workspace, float* out, void* stream);

/* The rays_rgba batching table of nerf/train_nerf.py:78-82 built on the device: row image*H*W + pixel =
 * (rays_o, rays_d of get_rays(width, height, focal, pose[image]), r, g, b, a); white_bkgd != 0 composites rgb on
 * white first (rgb*a + 1 - a, train_nerf.py:64-68).  poses [images,12] = c2w[:3,:4] row-major (device),
 * rgba [images,height,width,4] (device); out rays_rgba [images*height*width,10].  compute_f64 as in mi_gen_rays:
 * nonzero when the script's focal is an np.float64 scalar (nerf/data_loader.py:151 returns one), which makes
 * NumPy >= 2 evaluate get_rays in fp64 before train_nerf.py:84 rounds to fp32. */
int mi_ray_bank(int width, int height, double focal, const float* poses, const float* rgba, int white_bkgd,
                int64_t images, float* rays_rgba, int compute_f64, void* stream);

/* One optimiser step of torch.optim.Adam(betas, eps; no weight decay, no amsgrad) - nerf/train_nerf.py:98,168 - on the
 * parameters of 1 or 2 fields, fused with the refresh of their packed weight streams: every tensor's (param, exp_avg,
 * exp_avg_sq) is updated in place and each new parameter value is written to the positions of the field's forward
 * stream (mi_field_pack layout) and, when packed_bwd[f] is non-null, its transposed stream (mi_field_pack_bwd) that
 * hold it.  kinds[n_fields]; params / grads / exp_avg / exp_avg_sq / numel: one entry per tensor, field 0's
 * mi_field_num_params(kind) tensors first, in mi_field_pack order.  The scalars are torch's, computed by the caller in
 * double: step_size = -lr / (1 - beta1^t), bias_correction2_sqrt = sqrt(1 - beta2^t).  The streams must already
 * hold the current parameters (their padding entries are not rewritten). */
int mi_adam_step(int n_fields, const int* kinds, float* const* params, const float* const* grads, float* const* exp_avg,
                 float* const* exp_avg_sq, const int64_t* numel, float step_size, float one_minus_beta1, float beta2,
                 float one_minus_beta2, float eps, float bias_correction2_sqrt, float* const* packed_fwd,
                 float* const* packed_bwd, void* stream);

/* ---- marching cubes (mesh_stages.hip): the mesh half of create_mesh, pi_GAN/utils.py:109-180 ---------
 * skimage.measure.marching_cubes_lewiner(volume, level, spacing, gradient_direction, allow_degenerate=True) on a
 * C-contiguous fp32 device volume [nx, ny, nz] (nz fastest); every axis >= 2.  Two calls on one stream, one workspace
 * of mi_mc_workspace_bytes (needs no GPU; about 2 bytes per voxel):
 *   mi_marching_cubes_count  sweeps the volume, returns the vertex and triangle counts (synchronises the stream);
 *                            MI_ERANGE when level is outside [min, max] of the volume, MI_EINVAL when V >= 2^31;
 *   mi_marching_cubes_emit   with the same volume, level and workspace: verts[V,3] (f32, axis order of the volume,
 *                            times spacing[3]), faces[F,3] (int32), normals[V,3], values[V].  descent != 0 gives
 *                            skimage's default winding, 0 its 'ascent' winding.
 * The output is identical from run to run: vertices in order of owning voxel then axis, triangles in order of cube. */
int64_t mi_mc_workspace_bytes(int64_t nx, int64_t ny, int64_t nz);
int mi_marching_cubes_count(const float* volume, int64_t nx, int64_t ny, int64_t nz, double level, void* workspace,
                            int64_t* n_verts, int64_t* n_faces, void* stream);
int mi_marching_cubes_emit(const float* volume, int64_t nx, int64_t ny, int64_t nz, double level, const double* spacing,
                           int descent, void* workspace, float* verts, int* faces, float* normals, float* values,
                           void* stream);

/* ---- occupancy grids ------------------------------------------------------------------ */

/* A per-scene occupancy grid is one bit per cell of a dims[0] x dims[1] x dims[2] grid over an axis-aligned box: which cells
 * can hold density.  Cell (ix, iy, iz) has index (ix * dims[1] + iy) * dims[2] + iz and lives in word index >> 5, bit
 * index & 31 of a uint32 array of mi_occupancy_words(dims) words.  dims: HOST, 3 ints, each >= 1, product below 2^31 (else
 * MI_EINVAL; the two size queries need no GPU).  These calls BUILD such a grid from a field; "rendering with a grid" below
 * reads one.
 * mi_occupancy_cell_points: the supersample^3 (1..8 per axis) regular sub-sample points of cells [head, head + count) in
 * index order, points [count * supersample^3, 6] with a zero direction (sigma does not depend on it), ready for
 * mi_field_eval_points; with k = supersample, sub-sample (i, j, l) of the c-th cell of the range is row
 * c * k^3 + (i * k + j) * k + l and sits at lo + (cell index + (i + 0.5) / k) * cell along each axis, every operation
 * rounded on its own in fp32 (lo, cell: HOST, 3 floats each - the box's lower corner and a cell's edge lengths).
 * mi_occupancy_pack: from sigma [cells * supersample^3] in that order, a cell is occupied iff any of its sub-samples has
 * sigma > threshold (strict; a NaN is not above anything); the result is dilated `dilate` times by the 6-neighbourhood,
 * clipped at the box, and packed into bits (spare bits of the last word 0).  workspace:
 * mi_occupancy_pack_workspace_bytes(dims, dilate) device bytes; workspace_bytes = what the caller really provided. */
int64_t mi_occupancy_words(const int* dims);
int64_t mi_occupancy_pack_workspace_bytes(const int* dims, int dilate);
int mi_occupancy_cell_points(const int* dims, const float* lo, const float* cell, int supersample, int64_t head, int64_t count,
                             float* points, void* stream);
int mi_occupancy_pack(const float* sigma, const int* dims, int supersample, float threshold, int dilate, uint32_t* bits,
                      void* workspace, int64_t workspace_bytes, void* stream);

/* ---- a live grid: jittered partial updates of a per-cell density -------------------------
 *
 * A grid that follows a field while it trains keeps a float density per cell on the device (density [cells], all +0 at the
 * start) next to its bits.  One update re-samples a subset of the cells at one jittered point each, folds the new sigma in
 * with max(old * decay, new) and re-thresholds the density into the bits in place.  Nothing is read back by any of the calls.
 *
 * Random words: P(seed, R, j) is the Philox4x32-10 block with counter (R_lo, R_hi, j, 0) and key (seed_lo, seed_hi); word w of
 * stream R is word w & 3 of block w >> 2 (the words of mi_sample_coarse, whose stream is the ray).
 *
 * mi_occupancy_draw_points: rows [row0, row0 + count) of update number `epoch`.  Row r reads stream R = (epoch << 32) | r.
 * Its jitter is u_d = float(word_d >> 8) * 2^-24 for d = 0, 1, 2.  Its cell: mode 0 (sweep): cell = r (row0 + count <= cells);
 * mode 1 (draw): rows r < n_uniform take cell = (word_3 * cells) >> 32 in 64-bit arithmetic, the other rows take the first of
 * the candidates c_a = (word_{4+a} * cells) >> 32, a = 0..7, whose bit is set in bits, and c_7 if none is (no compaction, no
 * atomic).  Its point is lo_d + (float(i_d) + u_d) * cell_d with (i_0, i_1, i_2) the cell's coordinates, the add, the multiply
 * and the add each rounded on their own (at u = 1 - 2^-24 the inner sum may round up to i_d + 1: the far face of the cell);
 * the direction is 0.  Outputs: cell_ids [count] (device ints) and points [count, 6], ready for mi_field_eval_points.  lo,
 * cell: HOST, as for mi_occupancy_cell_points.  bits may be NULL when no row reads it (mode 0, or n_uniform >= row0 + count).
 * row0 + count must not exceed 2^31.
 *
 * mi_occupancy_density_update: the fold, over ALL rows of one update in one call (a cell sampled in two calls would decay
 * twice).  v_i = sigma_i > 0 ? sigma_i : +0 (so -0.0, negatives and NaN count as +0); m_c = the maximum of v_i over the rows
 * with cell_ids[i] == c; a cell with at least one row gets density_c = fmaxf(density_c * decay, m_c), the product rounded on
 * its own; every other cell keeps its bits.  The maximum is an integer atomic maximum on the floats' bits, so the result does
 * not depend on the order of arrival.  decay in [0, 1].  A row whose cell id lies outside the grid is ignored.
 *
 * mi_occupancy_density_pack: mean = float(sum of density in fp64 / cells), summed in a fixed order (the same bits in every
 * run); thr = relative ? fminf(threshold, mean) : threshold; a cell is occupied iff density > thr (strict); the result is
 * dilated and packed into bits as by mi_occupancy_pack.  mean and thr stay on the device.
 *
 * workspace: mi_occupancy_density_workspace_bytes(dims, dilate) device bytes - 4 bytes per cell of scratch ints, 8 bytes per
 * 4096 cells of partial sums (each of the two rounded up to whole 256-byte blocks), 256 bytes for mean and thr, and the byte
 * planes of mi_occupancy_pack_workspace_bytes(dims, dilate).  The update needs the size for dilate = 0, so one buffer sized
 * for the pack serves both.  Bad dims, null pointers, count < 0, a decay outside [0, 1] (or NaN), dilate < 0, rows past the
 * grid (mode 0) or past 2^31 and a short workspace: MI_EINVAL before any launch.  count == 0 launches nothing and returns 0. */
int mi_occupancy_draw_points(const uint32_t* bits, const int* dims, const float* lo, const float* cell, uint64_t seed,
                             uint32_t epoch, int mode, int64_t row0, int64_t count, int64_t n_uniform, int* cell_ids,
                             float* points, void* stream);
int64_t mi_occupancy_density_workspace_bytes(const int* dims, int dilate);
int mi_occupancy_density_update(const float* sigma, const int* cell_ids, int64_t count, const int* dims, float decay,
                                float* density, void* workspace, int64_t workspace_bytes, void* stream);
int mi_occupancy_density_pack(const float* density, const int* dims, float threshold, int relative, int dilate, uint32_t* bits,
                              void* workspace, int64_t workspace_bytes, void* stream);

/* ---- rendering with a grid (inference; NeRF, SirenNeRF, TinyNeRF) ------------------------
 *
 * The one rule: with a grid, a sample whose point lies in an unoccupied cell, or outside the box [lo, hi), has
 * raw = {0, 0, 0, 0} instead of the field's value; everything else is mi_render_rays.  The point is the fused forward's
 * p = o + d * z, for this rule with a rounded multiply, then a rounded add; it is placed by t = (p - lo) * inv_cell (a
 * rounded subtract, then a rounded multiply; lo, inv_cell: HOST, 3 floats each, inv_cell = cells per unit length), is inside
 * iff 0 <= t < dims on every axis (a NaN is not inside), and its cell is floor(t).
 *
 * mi_occupancy_mark_rays: the samples of rays [n,2,3] at depths z [n,S] that are occupied, as point indices ray * S + k
 * appended in any order to list [n*S] (device ints) and counted in the device int *count, which the call clears first.
 * raw [n,S,4], when not NULL, gets the rows of the unoccupied samples zeroed; occupied rows are not touched.  n * S must
 * fit an int (else MI_EINVAL, before any launch).
 *
 * mi_field_eval_rays_list: the field at the listed points alone - raw[list[e]] for e < *count has mi_field_eval_rays' bits,
 * no other row is written.  list entries are point indices in [0, n*S); FiLM kinds: MI_EINVAL.  The launch is sized for
 * n * S points from host values (no read-back; stream capture works).
 *
 * mi_render_rays_occupancy: mi_render_rays (one group, no film) under the rule above: sample_coarse, mark, list forward,
 * composite, sample_fine, mark, list forward, composite.  The coarse outputs are optional as there.  evaluated: optional
 * device int[2], the number of samples the coarse and the fine pass evaluated.  workspace: mi_render_workspace_bytes(n, Nc,
 * Nf) + mi_render_occupancy_extra_bytes(n, Nc, Nf) bytes (one list of n * (Nc + Nf) ints, used by both passes, and the
 * two counts); n * (Nc + Nf) must fit an int.  Both passes evaluate whole forwards of their listed points: the windowed
 * sigma-only coarse pass, the deferred colour branch and the shared-field merge of mi_render_rays are not combined with a
 * grid. */
int mi_occupancy_mark_rays(const uint32_t* bits, const int* dims, const float* lo, const float* inv_cell, const float* rays,
                           const float* z, int64_t n, int n_samples, int* list, int* count, float* raw, void* stream);
int mi_field_eval_rays_list(int kind, const float* packed, const float* rays, const float* z, int64_t n, int n_samples,
                            const int* list, const int* count, float* raw, void* stream);
int64_t mi_render_occupancy_extra_bytes(int64_t n, int n_coarse, int n_fine);
int mi_render_rays_occupancy(int kind_coarse, const float* packed_coarse, int kind_fine, const float* packed_fine,
                             const float* rays, int64_t n, float near_, float far_, int n_coarse, int n_fine,
                             const float* z_lin, const float* u_lin, const float* t_rand, uint64_t seed, uint64_t ray0,
                             const uint32_t* bits, const int* dims, const float* lo, const float* inv_cell, float* rgb_c,
                             float* depth_c, float* acc_c, float* rgb_f, float* depth_f, float* acc_f, int* evaluated,
                             void* workspace, int64_t workspace_bytes, void* stream);

/* ---- training with a grid (NeRF, SirenNeRF, TinyNeRF) -------------------------------------
 *
 * The rule above, differentiated: a listed sample contributes to the parameter gradients exactly what it contributes without
 * a grid, an unlisted sample (raw = 0, a constant) contributes nothing; the composite's backward runs on the full [n,S,4]
 * raw, zeros included.  A cell that is empty in the grid therefore gets no gradient and cannot fill up until the caller
 * rebuilds the grid: warm-up steps without a grid, dilation and the rebuild period are the caller's policy.
 *
 * mi_occupancy_mark_rays_ordered: mi_occupancy_mark_rays with the list in ASCENDING order of the point index, written without
 * atomics (a count per workgroup, a scan, a scatter), so that the list - the row order of the weight-gradient sums - is the
 * same in every run.  Same zeroing of raw, same count.  list needs room for mi_occupancy_ordered_list_ints(n, S) ints: the
 * n * S entries, then one scan slot per workgroup of 4096 points.
 *
 * mi_field_eval_rays_list_train: mi_field_eval_rays_list that keeps the layer inputs.  raw[list[e]] has
 * mi_field_eval_rays_train's bits; the saved rows of entry e are written at ROW e of every region of acts
 * (mi_field_train_acts_floats(kind) * n * S floats: compact rows, regions at the stride of the capacity n * S), with the
 * bits of that call's row list[e].  Rows at and past *count are not written.
 *
 * mi_field_backward_list: mi_field_backward over those compact rows: rows [0, *count) of acts, raw and g_raw [capacity,4]
 * read at rows list[e], dA rows e in grads_ws (mi_field_train_grads_floats(kind) * capacity floats), partial_ws of
 * mi_field_bwd_partial_floats_kind(kind, capacity) floats.  Every launch is sized from the capacity; the row count is read
 * on the device.  The weight-gradient kernels plan their number of slabs from the capacity, as mi_field_backward does for
 * that many points, and cut the rows they have into that many equal slabs: slab length = ceil(count / slabs) rounded up to
 * a multiple of 32.  grad_params are overwritten; with *count == 0 they are exactly 0.
 *
 * mi_render_rays_occupancy_train / _backward: mi_render_rays_occupancy's sequence with the ordered mark and the list forward
 * that keeps layer inputs, and the gradients of every parameter from the six output cotangents (NULL = zero; a pass without
 * any cotangent is skipped).  All six outputs are required.  One range per pass, nothing recomputed: workspace =
 * mi_render_workspace_bytes + mi_render_occupancy_train_extra_bytes (the same region behind the workspace as at inference,
 * but with an ordered list per pass, scan slots included, where inference has one list for both: the backward reads both
 * lists), saved = mi_render_occupancy_train_saved_bytes (both passes' compact rows at worst-case capacity), bwd_workspace =
 * mi_render_occupancy_backward_workspace_bytes; a caller with more rays than its memory allows cuts the rays into calls.
 * shared != 0: one field for both passes (packed_bwd_fine and grad_params_fine are not read); both passes run as passes of
 * that field over all their listed points and the two gradient sums are added into grad_params_coarse.  fields_written:
 * MI_WROTE_COARSE | MI_WROTE_FINE.  FiLM kinds, n * (Nc + Nf) past an int, short buffers and (forward) grid
 * bits that the runtime knows as memory of another device than the current one: MI_EINVAL before any launch. */
int64_t mi_occupancy_ordered_list_ints(int64_t n, int n_samples);
int mi_occupancy_mark_rays_ordered(const uint32_t* bits, const int* dims, const float* lo, const float* inv_cell,
                                   const float* rays, const float* z, int64_t n, int n_samples, int* list, int* count,
                                   float* raw, void* stream);
int mi_field_eval_rays_list_train(int kind, const float* packed, const float* rays, const float* z, int64_t n, int n_samples,
                                  const int* list, const int* count, float* raw, float* acts, void* stream);
int mi_field_backward_list(int kind, const float* packed_bwd, const float* acts, float* grads_ws, const float* raw,
                           const float* g_raw, const int* list, const int* count, int64_t capacity, float* partial_ws,
                           float* const* grad_params, void* stream);
int64_t mi_render_occupancy_train_extra_bytes(int64_t n, int n_coarse, int n_fine);
int64_t mi_render_occupancy_train_saved_bytes(int kind_coarse, int kind_fine, int64_t n, int n_coarse, int n_fine);
int64_t mi_render_occupancy_backward_workspace_bytes(int kind_coarse, int kind_fine, int shared, int64_t n, int n_coarse,
                                                     int n_fine);
int mi_render_rays_occupancy_train(int kind_coarse, const float* packed_coarse, int kind_fine, const float* packed_fine,
                                   const float* rays, int64_t n, float near_, float far_, int n_coarse, int n_fine,
                                   const float* z_lin, const float* u_lin, const float* t_rand, uint64_t seed, uint64_t ray0,
                                   const uint32_t* bits, const int* dims, const float* lo, const float* inv_cell, float* rgb_c,
                                   float* depth_c, float* acc_c, float* rgb_f, float* depth_f, float* acc_f, int* evaluated,
                                   void* workspace, int64_t workspace_bytes, void* saved, int64_t saved_bytes, void* stream);
int mi_render_rays_occupancy_backward(int kind_coarse, const float* packed_bwd_coarse, int kind_fine,
                                      const float* packed_bwd_fine, int shared, const float* rays, int64_t n, int n_coarse,
                                      int n_fine, const void* workspace, int64_t workspace_bytes, const void* saved,
                                      int64_t saved_bytes, const float* g_rgb_c, const float* g_depth_c, const float* g_acc_c,
                                      const float* g_rgb_f, const float* g_depth_f, const float* g_acc_f,
                                      float* const* grad_params_coarse, float* const* grad_params_fine, void* bwd_workspace,
                                      int64_t bwd_workspace_bytes, int* fields_written, void* stream);

/* ---- gradients to the rays with a grid (NeRF, SirenNeRF, TinyNeRF): opt-in, used by mirender/pose.py ---------------
 *
 * The rule: with a grid an unlisted sample's raw is the constant 0, so it sends nothing to the rays through the field; in the
 * composite its sigma = 0 gives an exact 0 in dL/d|d| (mi_composite_bwd_rays runs on the full [n,S,4] raw, zeros included).
 * A listed sample sends the rays exactly what it sends without a grid: g_o += g_pos, g_d += z_s g_pos + (I - v v^T) / |d| g_dir.
 * Occupancy is piecewise constant in the rays, and so are the clipped bounds: neither carries a gradient, and the depths carry
 * none either, as without a grid.
 *
 * mi_field_input_grad_rays_list: mi_field_input_grad_rays over the COMPACT rows a mi_field_backward_list call left behind
 * (same kind / acts / grads_ws / list / count / capacity; `params` as in mi_field_input_grad).  Ray r's samples are the run
 * [e0, e1) of the ascending list with r * n_samples <= list[e] < (r + 1) * n_samples, found on the device from *count (no
 * read-back); entry e reads row e of every region, z[list[e]] and ray r.  Rows and list entries at and past *count are never
 * read.  A ray with an empty run gets zeros (accumulate = 0) or keeps what it holds.  One wave owns a ray, no atomics.
 * FiLM kinds, a NULL pointer, n * n_samples past an int and capacity != n * n_samples: MI_EINVAL before any launch.
 *
 * mi_render_rays_occupancy_backward_rays: mi_render_rays_occupancy_backward (same arguments, same launches, same parameter
 * gradients bit for bit) that also writes dL/d(rays).  params_coarse / params_fine: HOST arrays of the fields' parameter
 * tensors (device pointers, state-dict order; with shared != 0 params_fine is not read).  g_rays [n,2,3] is OVERWRITTEN in
 * full whatever cotangents are NULL (all NULL: zeros); within it the sum runs composite coarse, field coarse, composite fine,
 * field fine.  It reads z from the workspace, so it serves the clipped training forward unchanged.  No workspace beyond
 * mi_render_rays_occupancy_backward's. */
int mi_field_input_grad_rays_list(int kind, const float* const* params, int n_params, const float* acts, const float* grads_ws,
                                  const int* list, const int* count, int64_t capacity, const float* rays, const float* z,
                                  int64_t n, int n_samples, int accumulate, float* g_rays, void* stream);
int mi_render_rays_occupancy_backward_rays(int kind_coarse, const float* packed_bwd_coarse, int kind_fine,
                                           const float* packed_bwd_fine, int shared, const float* rays, int64_t n, int n_coarse,
                                           int n_fine, const void* workspace, int64_t workspace_bytes, const void* saved,
                                           int64_t saved_bytes, const float* g_rgb_c, const float* g_depth_c, const float* g_acc_c,
                                           const float* g_rgb_f, const float* g_depth_f, const float* g_acc_f,
                                           float* const* grad_params_coarse, float* const* grad_params_fine, void* bwd_workspace,
                                           int64_t bwd_workspace_bytes, int* fields_written, const float* const* params_coarse,
                                           int n_params_coarse, const float* const* params_fine, int n_params_fine, float* g_rays,
                                           void* stream);

/* ---- clipping each ray's sampling range to the grid (NeRF, SirenNeRF, TinyNeRF) -----------
 *
 * The grid calls above decide WHETHER a sample is evaluated; these decide WHERE samples are placed.  The rule, for rays
 * [n,2,3], scalars near_ < far_, a grid, probes = M in [1, 4096] and pad >= 0, every operation in fp32 and rounded on its own:
 *   h = (far_ - near_) / float(M);  probe k in [0, M) sits at depth t_k = near_ + (float(k) + 0.5f) * h; its point is the mark
 *   rule's p = o + d * t_k and it is occupied exactly as mi_occupancy_mark_rays decides it (a NaN is outside).
 *   With k0 / k1 the least / greatest occupied probe: a = max(k0 - pad, 0), b = min(k1 + 1 + pad, M),
 *   near_r = near_ + float(a) * h,  far_r = (b == M) ? far_ : near_ + float(b) * h.
 *   A ray without an occupied probe keeps (near_, far_); the mark then culls its samples as it does without clipping.
 * A structure thinner than h between two probes can be missed: probes and pad are the caller's, as a grid's resolution and
 * dilation are.  A step of at most half a cell along the ray is a sound default.
 *
 * mi_occupancy_clip_rays: bounds [n,2] (device floats) = (near_r, far_r) of every ray.  One wave per ray; no read-back.
 *
 * mi_sample_coarse_bounds / mi_sample_fine_bounds: mi_sample_coarse / mi_sample_fine_pos with their arithmetic unchanged and
 * the coarse linspace evaluated in the kernel over the ray's own range, lin(i) = linspace(bounds[r][0], bounds[r][1], Nc)[i]
 * (ATen's scalar formula).  A z_lin table has no meaning per ray: they take none.  Bounds equal to (near_, far_) on every ray
 * give the bits of the scalar calls with z_lin = NULL; ray r of a bounds call has the bits of the scalar call on that one ray
 * with (near_r, far_r) and ray0 + r.  z_samples and pos are optional (NULL), as in mi_sample_fine_pos.
 *
 * mi_render_rays_occupancy_clip / _clip_train: mi_render_rays_occupancy / _train with probes, pad in place of z_lin: the clip
 * first, then the same sequence with the two bounds samplers.  workspace: the unclipped call's bytes +
 * mi_render_occupancy_clip_extra_bytes(n) (the bounds, align64(2 n) floats, BEHIND the unclipped call's regions:
 * mi_render_rays_occupancy_backward, which reads z from the workspace and takes no near / far, serves the clipped training
 * forward unchanged and accepts its larger workspace).  probes outside [1, 4096], pad < 0, !(near_ < far_), a NULL bounds, a
 * short workspace, FiLM kinds and the grid checks: MI_EINVAL before any launch. */
int mi_occupancy_clip_rays(const uint32_t* bits, const int* dims, const float* lo, const float* inv_cell, const float* rays,
                           int64_t n, float near_, float far_, int probes, int pad, float* bounds, void* stream);
int mi_sample_coarse_bounds(int64_t n, const float* bounds, int n_coarse, const float* t_rand, uint64_t seed, uint64_t ray0,
                            float* z, void* stream);
int mi_sample_fine_bounds(int64_t n, const float* bounds, int n_coarse, int n_fine, const float* u_lin, const float* z_coarse,
                          const float* weights, float* z_samples, float* z_fine, int* pos, void* stream);
int64_t mi_render_occupancy_clip_extra_bytes(int64_t n);
int mi_render_rays_occupancy_clip(int kind_coarse, const float* packed_coarse, int kind_fine, const float* packed_fine,
                                  const float* rays, int64_t n, float near_, float far_, int n_coarse, int n_fine, int probes,
                                  int pad, const float* u_lin, const float* t_rand, uint64_t seed, uint64_t ray0,
                                  const uint32_t* bits, const int* dims, const float* lo, const float* inv_cell, float* rgb_c,
                                  float* depth_c, float* acc_c, float* rgb_f, float* depth_f, float* acc_f, int* evaluated,
                                  void* workspace, int64_t workspace_bytes, void* stream);
int mi_render_rays_occupancy_clip_train(int kind_coarse, const float* packed_coarse, int kind_fine, const float* packed_fine,
                                        const float* rays, int64_t n, float near_, float far_, int n_coarse, int n_fine,
                                        int probes, int pad, const float* u_lin, const float* t_rand, uint64_t seed,
                                        uint64_t ray0, const uint32_t* bits, const int* dims, const float* lo,
                                        const float* inv_cell, float* rgb_c, float* depth_c, float* acc_c, float* rgb_f,
                                        float* depth_f, float* acc_f, int* evaluated, void* workspace, int64_t workspace_bytes,
                                        void* saved, int64_t saved_bytes, void* stream);

/* ---- measurement hooks (bench.py) ---------------------------------------------------- */

/* HIP events owned by the library's HIP runtime (the one the kernels launch on), so a host
 * program can time individual launches without linking HIP itself.  mi_event_elapsed_ms
 * synchronises on `stop`. */
void* mi_event_create(void);
void mi_event_destroy(void* ev);
int mi_event_record(void* ev, void* stream);
int mi_event_elapsed_ms(void* start, void* stop, float* ms);
/* While set (thread-local; pass NULLs to clear), mi_render_rays records these events on its
 * stream immediately before/after the coarse and the fine field-MLP launch. */
void mi_render_set_mlp_events(void* start_coarse, void* stop_coarse, void* start_fine, void* stop_fine);

/* ---- test hooks of the deferred colour branch ---------------------------------------- */

/* mi_field_eval_rays with the colour branch deferred to the points with sigma > 0 (NeRF and TinyNeRF, else MI_EINVAL; film
 * is ignored): raw [n,S,4] has mi_field_eval_rays' bits wherever sigma > 0 and r = g = b = 0 elsewhere (sigma: its bits
 * everywhere).  extra: a device buffer of mi_render_deferred_colour_extra_bytes(n, Nc, Nf) bytes for any Nc + Nf = n_samples,
 * Nf > 0; extra_bytes = what the caller really provided. */
int mi_field_eval_rays_deferred(int kind, const float* packed, const float* film, const float* rays, const float* z,
                                int64_t n_groups, int64_t rays_per_group, int n_samples, float* raw, void* extra,
                                int64_t extra_bytes, void* stream);
/* Points per chunk of the deferred colour branch (process-wide; 0 = the build's constant, 2^22): a debug hook, so that a
 * test can force several chunks at small sizes.  mi_render_deferred_colour_extra_bytes follows it. */
void mi_render_set_colour_chunk_rows(int64_t rows);

#ifdef __cplusplus
}
#endif
#endif /* MI_RENDER_H */
