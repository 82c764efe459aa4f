// mi_device.h - what kernel code of libmirender shares (gfx950 only) and nothing else: a device helper, the kernel argument
// structs of the fused field MLP and the stamp macro.  Host plumbing is in mi_host.h, the launcher declarations in launchers.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>
#include <utility>

namespace mi {

template <class F, int... I>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
// f(integral_constant<int,0>) ... f(integral_constant<int,N-1>), fully unrolled at compile time
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    static_for_impl(static_cast<F&&>(f), std::make_integer_sequence<int, N>{});
}

// arguments of the fused field-MLP kernels (field_mlp_*.hip; launched by field_mlp.hip)
struct MlpArgs {
    const float* packed;    // packed weight stream (field_layout.h)
    const float* film;      // [groups][film_depth + 1][512] or null
    const float* a;         // points x[M,6] (mode 0) or rays [N,2,3] (mode 1)
    const float* z;         // [N,S] (mode 1)
    float* out;             // [M,4]; the sigma-only forward: [M] (sigma alone)
    int64_t points_per_group;
    int64_t rays_per_group;
    int64_t tiles_per_group;
    int n_samples;
    int mode;
    float* save;            // training: saved layer inputs, region r = save + act_offset(r) * save_points
    int64_t save_points;    // points in this launch (row count of every saved region)
    unsigned long long* stamps;   // diagnostic build (-DMI_PROFILE_STAMPS) only: [block][128] s_memtime values
    int film_depth;         // FiLM kinds: hidden_layers (wave-uniform; the run-time-depth instances read it), else 0
    // windowed sigma-only forward (launch_mlp_window): samples [win_k0, win_k0 + 2^win_log2) of the rays in a live list
    // (the list-driven forward, launch_mlp_list, keeps its list of POINT indices and that list's count in the same two fields)
    const int* live_rays;   // [live count] ray indices, any order; null = rays 0..n_rays-1
    const int* live_count;  // device count of live_rays; null = n_rays
    int64_t n_rays;         // rays of the call (the worst-case live count the grid is sized for)
    int win_k0;
    int win_log2;
};

// The live list of one chunk of the fine pass (DeferredColourBuf, render_path.h): the trunk-and-spill instance appends to it, the colour-branch
// kernel reads it.  Point indices are relative to the launch's a.out / a.z (the chunk's first point is 0).
struct DeferArgs {
    float* rows;            // [entries][256] H8 (the last trunk layer's activation) of the listed points
    int* idx;               // [entries] point index of each entry
    int* count;             // entries; cleared before the trunk-and-spill launch
};

// In-kernel cycle stamps for the diagnostic build (csrc/build.py --profile -> gpurun_tools/libmirender_prof.so);
// the product build compiles them out.
#ifdef MI_PROFILE_STAMPS
#define MI_STAMP(a, i) do { if (threadIdx.x == 0 && (a).stamps) (a).stamps[(int64_t)blockIdx.x * 128 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define MI_STAMP(a, i) do { } while (0)
#endif

// The two packed weight streams of a field kind (field_layout.h): forward order, and transposed for the backward chain.
enum StreamDir : int { STREAM_FWD = 0, STREAM_BWD = 1 };

}  // namespace mi
