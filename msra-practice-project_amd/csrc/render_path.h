// render_path.h - what the host units of the render paths share: api.hip (the one-stage wrappers), render_path.hip
// (mi_render_rays), train_path.hip (mi_render_rays_train / _backward) and occupancy_path.hip (the grid-driven calls).  Host
// arithmetic only: no kernel unit includes it, so an edit here compiles these four units and none of the kernels.
//   - the workspace layouts and the region allocator;
//   - the descriptor of a call, the fine pass's plan and the coarse-to-fine sequence, stated once (run_render_passes);
//   - the checks and helpers that more than one path uses.
#pragma once
#include "../../include/mi_render.h"
#include "field_kinds_host.h"
#include "launchers.h"

namespace mi {

// The workspace of mi_render_rays / mi_render_rays_train for n rays of Nc + Nf samples: the five regions of
// mi_render_workspace_bytes, then the three that one field for both passes adds (mi_render_shared_field_extra_bytes) - or,
// in their place, what two fields' deferred colour branch adds (DeferredColourBuf below, mi_render_deferred_colour_extra_bytes).
struct RenderWorkspace {
    struct Regions {
        float *z_c, *raw_c, *w_c, *z_f, *raw_f;       // [n,Nc] [n,Nc,4] [n,Nc] [n,S] [n,S,4]
        float *z_s, *raw_s;                           // [n,Nf] [n,Nf,4]
        int* pos;                                     // [n,S]
    };
    static constexpr int kBase = 5, kAll = 8;
    int64_t floats[kAll];
    RenderWorkspace(int64_t n, int nc, int nf)
        : floats{n * nc, n * nc * 4, n * nc, n * ((int64_t)nc + nf), n * ((int64_t)nc + nf) * 4,
                 n * nf, n * nf * 4, n * ((int64_t)nc + nf)} {}
    int64_t bytes(int first, int last) const {
        int64_t f = 0;
        for (int i = first; i < last; ++i) f += align64(floats[i]);
        return f * (int64_t)sizeof(float);
    }
    int64_t base_bytes() const { return bytes(0, kBase); }
    int64_t shared_extra_bytes() const { return bytes(kBase, kAll); }
    // the shared-field regions lie behind base_bytes(): theirs to use only in a workspace that holds them
    Regions carve(void* base) const {
        float* p[kAll];
        float* ws = (float*)base;
        for (int i = 0; i < kAll; ++i) { p[i] = ws; ws += align64(floats[i]); }
        return {p[0], p[1], p[2], p[3], p[4], p[5], p[6], (int*)p[7]};
    }
};

// The buffer of the fine pass's deferred colour branch (mi_render_deferred_colour_extra_bytes), for n rays of S samples
// evaluated in chunks of whole rays of at most chunk_rows points (one ray where S is larger): the H8 rows [cap][256] and the
// point indices [cap] of one chunk's live list (worst case: every point of the chunk live), and one count per chunk.  In a
// render workspace it lies behind base_bytes(), where the shared-field regions lie: the two paths exclude each other.
struct DeferredColourBuf {
    struct Regions { float* rows; int* idx; int* counts; };
    int64_t chunk_rays, n_chunks, cap;
    DeferredColourBuf(int64_t n, int64_t S, int64_t chunk_rows) {
        chunk_rays = chunk_rows / (S > 0 ? S : 1);
        if (chunk_rays < 1) chunk_rays = 1;
        if (chunk_rays > n) chunk_rays = n;
        n_chunks = chunk_rays > 0 ? (n + chunk_rays - 1) / chunk_rays : 0;
        // A chunk uses chunk_rays * S rows.  Where that falls short of chunk_rows (S does not divide it) the buffer is still
        // sized for chunk_rows, so that its size is the documented min(n * S, chunk_rows) rows: slack of less than one ray.
        cap = chunk_rays * S;
        if (cap < chunk_rows) cap = chunk_rows < n * S ? chunk_rows : n * S;
    }
    int64_t bytes() const { return (align64(cap * 256) + align64(cap) + align64(n_chunks)) * (int64_t)sizeof(float); }
    Regions carve(void* base) const {
        float* rows = (float*)base;
        int* idx = (int*)(rows + align64(cap * 256));
        return {rows, idx, idx + align64(cap)};
    }
};

// Consecutive regions of a float workspace, each starting on a 64-float block: take(x) is the offset of the next x floats.
struct RegionAllocator {
    int64_t floats = 0;
    int64_t take(int64_t x) { const int64_t o = floats; floats += align64(x); return o; }
};

// ---- one call of a render path ------------------------------------------------------------------------------------------
// n = n_groups * rays_per_group rays of Nc coarse and Nf more fine samples; shared: one field serves both passes.
struct RenderCall {
    int64_t n_groups, rays_per_group, n;
    int Nc, Nf;
    bool shared;
    RenderCall(int64_t groups, int64_t rpg, int nc, int nf, bool one_field)
        : n_groups(groups), rays_per_group(rpg), n(groups * rpg), Nc(nc), Nf(nf), shared(one_field) {}
};

// the one-field rule: the same kind reading the same packed stream
inline bool one_field(int kind_coarse, const float* packed_coarse, int kind_fine, const float* packed_fine) {
    return kind_coarse == kind_fine && packed_coarse == packed_fine;
}

// What the fine pass has to evaluate.
//   FINE_IS_COARSE    one field, Nf = 0: sort(z_coarse) == z_coarse, so the second pass would re-evaluate identical inputs
//                     (render.py:140-145).  One composite writes the fine outputs; the coarse outputs asked
//                     for are copies of them.
//   FINE_NEW_SAMPLES  one field, Nf > 0: Nc of the fine pass's Nc + Nf points are the coarse pass's points - the field at the
//                     Nf new depths only, merged into sorted order (render_stages.hip: merge_raw_kernel).  Needs the
//                     workspace's shared-field regions (z_s, raw_s, pos).
//   FINE_WHOLE        the field at all Nc + Nf depths: two fields, or one field in a workspace without those regions (same
//                     results).
enum FinePlan { FINE_IS_COARSE, FINE_NEW_SAMPLES, FINE_WHOLE };
inline FinePlan fine_plan(bool shared, int nf, bool has_shared_regions) {
    if (shared && nf == 0) return FINE_IS_COARSE;
    return shared && has_shared_regions ? FINE_NEW_SAMPLES : FINE_WHOLE;
}

// What the coarse field step left in the workspace, which decides the coarse composite:
//   COARSE_RAW      raw rows [n,Nc,4] in raw_c: the composite with rgb_c, else the weights from the sigma channel;
//   COARSE_SIGMA    sigma [n,Nc], compact at the start of raw_c: the weights composite;
//   COARSE_WEIGHTS  w_c (and depth_c / acc_c where asked for) already written, by the windowed pass: no composite.
enum CoarseLeft { COARSE_RAW, COARSE_SIGMA, COARSE_WEIGHTS };

// the per-call values that the sequence hands on to its stages unchanged
struct RenderIO {
    const float* rays;
    float near_, far_;
    const float *z_lin, *u_lin, *t_rand;
    uint64_t seed, ray0;
    float *rgb_c, *depth_c, *acc_c, *rgb_f, *depth_f, *acc_f;     // the coarse three may be null
    // optional [n,2]: a sampling range per ray (mi_occupancy_clip_rays); both samplers then run over it, without near_ / far_ / z_lin
    const float* bounds = nullptr;
};

// one field with Nf = 0: the fine outputs and the coarse outputs are one composite's; copies it to every non-null dst
int copy_render_outputs(const char* fn, int64_t n, float* rgb_dst, float* depth_dst, float* acc_dst, const float* rgb_src,
                        const float* depth_src, const float* acc_src, hipStream_t stream);

// The coarse-to-fine sequence of every render path: sample coarse, coarse field, coarse composite (or weights), sample fine,
// fine field, merge (FINE_NEW_SAMPLES), fine composite.  The two field steps are the caller's: each is called once as
// step(z [n,samples], samples per ray, raw [n,samples,4]) -> rc, and `left` says what the coarse one leaves behind.
// Everything is already checked by the entry point; launches only, grids from host values (no read-back: graph-capturable).
template <class CoarseField, class FineField>
int run_render_passes(const char* fn, const RenderCall& C, FinePlan plan, const RenderIO& io, const RenderWorkspace::Regions& ws,
                      CoarseLeft left, CoarseField&& coarse_field, FineField&& fine_field, hipStream_t hs) {
    const int64_t n = C.n;
    const int nc = C.Nc, nf = C.Nf, S = nc + nf;
    int rc;
    // the one branch on io.bounds: which pair of samplers the sequence runs
    const auto sample_fine = [&](float* z_s, int* pos) {
        return io.bounds ? launch_sample_fine_bounds(n, io.bounds, nc, nf, io.u_lin, ws.z_c, ws.w_c, z_s, ws.z_f, pos, hs)
                         : launch_sample_fine(n, io.near_, io.far_, nc, nf, io.z_lin, io.u_lin, ws.z_c, ws.w_c, z_s, ws.z_f, pos, hs);
    };
    if ((rc = io.bounds ? launch_sample_coarse_bounds(n, io.bounds, nc, io.t_rand, io.seed, io.ray0, ws.z_c, hs)
                        : launch_sample_coarse(n, io.near_, io.far_, nc, io.z_lin, io.t_rand, io.seed, io.ray0, ws.z_c, hs))) return rc;
    if ((rc = coarse_field(ws.z_c, nc, ws.raw_c))) return rc;
    if (plan == FINE_IS_COARSE) {
        if ((rc = launch_composite(n, nc, ws.raw_c, ws.z_c, io.rays, io.rgb_f, io.depth_f, io.acc_f, ws.w_c, hs))) return rc;
        return copy_render_outputs(fn, n, io.rgb_c, io.depth_c, io.acc_c, io.rgb_f, io.depth_f, io.acc_f, hs);
    }
    if (left == COARSE_RAW && io.rgb_c) rc = launch_composite(n, nc, ws.raw_c, ws.z_c, io.rays, io.rgb_c, io.depth_c, io.acc_c, ws.w_c, hs);
    else if (left == COARSE_RAW) rc = launch_composite_weights(n, nc, ws.raw_c + 3, 4, ws.z_c, io.rays, io.depth_c, io.acc_c, ws.w_c, hs);   // raw's sigma channel
    else if (left == COARSE_SIGMA) rc = launch_composite_weights(n, nc, ws.raw_c, 1, ws.z_c, io.rays, io.depth_c, io.acc_c, ws.w_c, hs);
    if (rc) return rc;
    if (plan == FINE_NEW_SAMPLES) {
        if ((rc = sample_fine(ws.z_s, ws.pos))) return rc;
        if ((rc = fine_field(ws.z_s, nf, ws.raw_s))) return rc;
        if ((rc = launch_merge_raw(n, nc, nf, ws.raw_c, ws.raw_s, ws.pos, ws.raw_f, hs))) return rc;
    } else {
        if ((rc = sample_fine(nullptr, nullptr))) return rc;
        if ((rc = fine_field(ws.z_f, S, ws.raw_f))) return rc;
    }
    return launch_composite(n, S, ws.raw_f, ws.z_f, io.rays, io.rgb_f, io.depth_f, io.acc_f, nullptr, hs);
}

// ---- helpers of more than one path ---------------------------------------------------------------------------------------
// api.hip: one launch of a kind's fused forward, arguments already checked.  mode 0: a = points [n_groups * ppg, 6]; mode 1:
// a = rays, z [rays, S], ppg = rpg * S.  save: the training forward's layer inputs; sigma_only: the sigma-only instance.
int eval_field(int kind, const float* packed, const float* film, const float* a, const float* z, int64_t n_groups, int64_t ppg,
               int64_t rpg, int S, int mode, float* out, hipStream_t s, float* save = nullptr, bool sigma_only = false);
// ... over rays, as every path's field step calls it
inline int eval_field_rays(int kind, const float* packed, const float* film, const float* rays, const float* z, int64_t n_groups,
                           int64_t rpg, int S, float* raw, hipStream_t s, float* save = nullptr) {
    return eval_field(kind, packed, film, rays, z, n_groups, rpg * S, rpg, S, 1, raw, s, save);
}

// occupancy_path.hip.  occupancy_cells: dims >= 1 with a product below 2^31, the product, or 0 with the error set.
// occupancy_grid_args: the one place a caller's grid is checked (dims first, then the pointers) and copied into one.
// eval_rays_list: launch_mlp_list over one group of n rays x S samples; acts null = inference, else the saved rows' destination.
int64_t occupancy_cells(const char* fn, const int* dims);
int occupancy_grid_args(const char* fn, const uint32_t* bits, const int* dims, const float* lo, const float* inv_cell,
                        OccupancyGridArgs* grid);
// ... and the one place the arguments of a clip are: near_ < far_ (a NaN is refused), 1 <= probes <= 4096, pad >= 0
int occupancy_clip_args(const char* fn, float near_, float far_, int probes, int pad);
int eval_rays_list(int kind, const float* packed, const float* rays, const float* z, int64_t n, int S, const int* list,
                   const int* count, float* raw, float* acts, hipStream_t stream);

// train_path.hip: a scratch copy of a kind's parameter gradients (its floats; its tensors, out[2 * n_layers]); dst[i] += src[i]
int64_t param_floats(int kind);
void scratch_params(int kind, float* base, float** out);
int add_param_grads(int kind, float* const* dst, float* const* src, hipStream_t stream);

// render_path.hip: a field that receives gradients in a backward (`which`: "coarse" / "fine") has its transposed stream, its
// gradient array and every gradient pointer of its kind
int check_field_grads(const char* fn, const char* which, int kind, const float* packed_bwd, float* const* grads);

// the fields_written word of a backward: one field's gradients are the coarse field's, whichever pass asked for them
inline int fields_written_word(bool shared, bool coarse, bool fine, bool film) {
    return (shared || coarse ? MI_WROTE_COARSE : 0) | (!shared && fine ? MI_WROTE_FINE : 0) | (film ? MI_WROTE_FILM : 0);
}

}  // namespace mi
