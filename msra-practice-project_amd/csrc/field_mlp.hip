// field_mlp.hip - fused radiance-field MLP forward for gfx950 (MI355X).
//
// What it replaces: the `network(inputs[M,6]) -> [M,4]` call inside run_network
// (reference nerf/render.py:59-75) for NeRF / SirenNeRF (nerf/nerf.py:52-170), FilmSirenNeRF
// (pi_GAN/modules.py:70-118) and the build-defined TinyNeRF, including positional encoding
// (nerf/nerf.py:44-49), every Dense/Siren/FiLM layer, the sigma/rgb heads and - in ray mode -
// the point generation pts = o + d*z, view = d/|d| of render_rays (render.py:122,134).
//
// Structure (one workgroup = 4 waves = 128 points, one wave per SIMD, whole register file):
//   * features on MFMA rows, points on MFMA columns (v_mfma_f32_32x32x2_f32, exact fp32), so
//     the 8x16 accumulator registers of a 256-wide layer ARE the next layer's B operands:
//     activations never leave registers between layers;
//   * weights stream HBM/L2 -> LDS by global_load_lds_dwordx4 (1 KiB pieces) in the order the
//     MFMAs consume them (field_layout.h), double-buffered per 32-wide K block (32 KiB), one
//     barrier per K block; A fragments are ds_read_b128 (4 MFMAs per read);
//   * bias / head weights / K=3 input columns ride the same stream as 1 KiB VEC pieces into a
//     per-layer LDS aux slot; FiLM gamma|beta rows are DMA'd per image into a film slot;
//   * sigma / rgb heads (1 and 3 outputs) are VALU dot products + one cross-half shuffle.
// Roofline: fp32 MFMA (157 TFLOP/s); HBM traffic is 24-28 B in + 16 B out per point.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "field_kinds_host.h"
#include "field_mlp_device.h"
#include "field_mlp_instances.h"
#include "launchers.h"

namespace mi {

// ---- host side ---------------------------------------------------------------------------
// This unit is host code only.  The kernels live in one unit per family - field_mlp_nerf.hip (NeRF, TinyNeRF and the
// colour-branch kernel), field_mlp_siren.hip, field_mlp_film.hip - and each of those defines its rows of the table below
// (field_mlp_instances.h, with the variants).
// One table of instances, [row][variant].  Rows: the fixed kinds, then the run-time-depth FiLM instances without / with the
// direction (MI_FIELD_FILM_DEPTH kinds other than depth 8, which IS kinds 2 / 3).
// The FiLM kinds have no sigma-only instance (their caller, pi_GAN, renders both passes with one field and needs the
// coarse colours for the merge): has_sigma_only_kernel() is false for them.
constexpr int kFilmDepthRow = MI_FIELD_KINDS;      // + use_dir
static const void* const* const kKernels[MI_FIELD_KINDS + 2] = {
    kNerfRows[0],                  // MI_FIELD_NERF
    kSirenRow[0],                  // MI_FIELD_SIREN_NERF
    kFilmRows[0], kFilmRows[1],    // MI_FIELD_FILM_SIREN_NERF, ..._NODIR
    kNerfRows[1],                  // MI_FIELD_TINY_NERF
    kFilmRows[2], kFilmRows[3]};   // any depth, no dir; any depth, dir

bool has_deferred_colour_kernels(int kind) { return kind >= 0 && kind < MI_FIELD_KINDS && kKernels[kind][FWD_SPILL] && kKernels[kind][FWD_COLOUR]; }
bool has_sigma_only_kernel(int kind) { return kind >= 0 && kind < MI_FIELD_KINDS && kKernels[kind][FWD_SIGMA]; }
bool has_list_kernel(int kind) { return kind >= 0 && kind < MI_FIELD_KINDS && kKernels[kind][FWD_LIST] && kKernels[kind][FWD_LIST_SAVE]; }

// Every instance runs 256 threads on 148 KiB of dynamic LDS: the per-kernel limit is raised once per device (host-side
// attribute, no device work).
static int launch_instance(const void* fn, int64_t blocks, void* arg, hipStream_t stream, const char* what) {
    const size_t lds = kLdsFloats * sizeof(float);
    static PerDeviceOnce attr_once;
    const int arc = attr_once.run([&]() {
        for (const void* const* row : kKernels)
            for (int v = 0; v < FWD_VARIANTS; ++v) {
                const void* const f = row[v];
                if (!f) continue;
                const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
                if (e != hipSuccess) { set_error("hipFuncSetAttribute: %s", hipGetErrorString(e)); return -2; }
            }
        return 0;
    });
    if (arc) return arc;
    void* args[] = {arg};
    (void)hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(256), args, lds, stream);
    return check_launch(what);
}

int launch_mlp(int kind_in, const MlpArgs& a, int64_t n_groups, hipStream_t stream, bool sigma_only) {
    const int kind = canon_kind(kind_in);
    const int64_t blocks = n_groups * a.tiles_per_group;
    if (blocks <= 0) return 0;
    if (blocks > 0x7fffffffLL) { set_error("too many point tiles (%lld)", (long long)blocks); return -1; }
    if (bad_kind(kind)) return -1;
    if (sigma_only && (a.save || !has_sigma_only_kernel(kind))) {
        set_error("kind %d has no sigma-only forward%s", kind, a.save ? " with saved layer inputs" : "");
        return -1;
    }
    if (is_depth_kind(kind) && (a.film_depth != film_depth(kind) || !a.film)) {
        set_error("FiLM depth kind 0x%x launched without its depth or table", kind);
        return -1;
    }
    const int row = is_depth_kind(kind) ? kFilmDepthRow + film_use_dir(kind) : kind;
    return launch_instance(kKernels[row][sigma_only ? FWD_SIGMA : a.save ? FWD_SAVE : FWD_INFER], blocks, const_cast<MlpArgs*>(&a), stream,
                           "field_mlp_fwd");
}

int launch_mlp_window(int kind_in, const MlpArgs& a, hipStream_t stream) {
    const int kind = canon_kind(kind_in);
    if (bad_kind(kind)) return -1;
    if (a.save || a.film || !has_sigma_only_kernel(kind) || a.win_log2 < 0 || a.win_log2 > 7 || a.win_k0 < 0 ||
        a.win_k0 >= a.n_samples || a.n_rays > 0x7fffffffLL) {
        set_error("kind %d: bad windowed sigma-only launch", kind);
        return -1;
    }
    const int64_t per_tile = 128 >> a.win_log2;
    const int64_t blocks = (a.n_rays + per_tile - 1) / per_tile;        // worst case: every ray live
    if (blocks <= 0) return 0;
    if (blocks > 0x7fffffffLL) { set_error("too many point tiles (%lld)", (long long)blocks); return -1; }
    return launch_instance(kKernels[kind][FWD_SIGMA_WINDOW], blocks, const_cast<MlpArgs*>(&a), stream, "field_mlp_fwd_window");
}

int launch_mlp_list(int kind_in, const MlpArgs& a_in, const int* list, const int* count, hipStream_t stream) {
    const int kind = canon_kind(kind_in);
    if (bad_kind(kind)) return -1;
    if (!has_list_kernel(kind) || (a_in.save && a_in.save_points < a_in.points_per_group) || a_in.film || a_in.mode != 1 || a_in.n_samples < 1 || !list || !count ||
        a_in.points_per_group < 1 || a_in.points_per_group > 0x7fffffffLL ||
        a_in.points_per_group != a_in.rays_per_group * a_in.n_samples) {
        set_error("kind %d: bad list-driven launch", kind);
        return -1;
    }
    MlpArgs a = a_in;
    a.live_rays = list; a.live_count = count;
    const int64_t blocks = (a.points_per_group + 127) / 128;           // worst case: every point listed
    return launch_instance(kKernels[kind][a.save ? FWD_LIST_SAVE : FWD_LIST], blocks, &a, stream, "field_mlp_fwd_list");
}

// compute units of the current device, asked once per device ordinal (0 and the error set if the query fails)
static int compute_units() {
    static std::atomic<int> cached[256] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 256) { set_error("hipGetDevice failed"); return 0; }
    int cus = cached[dev].load(std::memory_order_relaxed);
    if (cus < 1) {
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) {
            set_error("field_mlp_colour: no compute-unit count");
            return 0;
        }
        cached[dev].store(cus, std::memory_order_relaxed);
    }
    return cus;
}

// shared checks of the two deferred-colour launches: a mode-1 launch of one group whose point indices fit the list's ints
static int check_deferred(int kind, const MlpArgs& a, const DeferArgs& d) {
    if (bad_kind(kind)) return -1;
    if (!has_deferred_colour_kernels(kind) || a.save || a.film || a.mode != 1 || a.n_samples < 1 || !d.rows || !d.idx || !d.count ||
        a.points_per_group < 1 || a.points_per_group > 0x7fffffffLL || a.tiles_per_group != (a.points_per_group + 127) / 128) {
        set_error("kind %d: bad deferred-colour launch", kind);
        return -1;
    }
    return 0;
}

int launch_mlp_trunk_spill(int kind, const MlpArgs& a, const DeferArgs& d, hipStream_t stream) {
    if (const int rc = check_deferred(kind, a, d)) return rc;
    DeferMlpArgs da{a, d};
    return launch_instance(kKernels[kind][FWD_SPILL], a.tiles_per_group, &da, stream, "field_mlp_trunk_spill");
}

int launch_mlp_colour(int kind, const MlpArgs& a, const DeferArgs& d, hipStream_t stream) {
    if (const int rc = check_deferred(kind, a, d)) return rc;
    // one block per CU (148 KiB of LDS each) strides over the tiles below the device count; never more blocks than tiles
    const int cus = compute_units();
    if (cus < 1) return -2;
    const int64_t blocks = a.tiles_per_group < cus ? a.tiles_per_group : cus;
    DeferMlpArgs da{a, d};
    return launch_instance(kKernels[kind][FWD_COLOUR], blocks, &da, stream, "field_mlp_colour");
}

}  // namespace mi
