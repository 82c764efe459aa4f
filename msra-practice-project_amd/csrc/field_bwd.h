// field_bwd.h - what the two translation units of the field backward share (gfx950): what autograd does for
// `network(inputs)` inside run_network (reference nerf/render.py:72-74) when train_nerf.py:168 / pi_GAN/train.py call
// loss.backward().
//
// Three kinds of kernels, all fp32, in two units:
//   field_bwd_chain.hip
//   1. backward CHAIN (one per field kind): same structure as the forward - 128 points per workgroup,
//      features on MFMA rows, the accumulators of dX_l = W_l^T dA_l are, after the activation derivative,
//      the B operands of the next (earlier) layer; transposed weights stream through LDS from a second
//      packed stream (field_layout.h build_*_bwd).  It reads the saved layer inputs for the activation
//      derivative and writes dA of every linear layer as [point][feature] rows.
//   field_bwd_dw.hip (with the host planner and the orchestration of a whole backward pass)
//   2. dW GEMM: dW_l[M,K] = sum_p dA_l[p,:]^T X_l[p,:] - a plain GEMM whose contraction is over POINTS.
//      Features sit on the MFMA lanes (one float4 load per lane gives the operands of four 32-wide blocks
//      straight from the row-major rows, no LDS), each workgroup reduces a slab of points into a full
//      256x256 tile held in accumulators (256 registers per lane), slabs are combined by a second kernel in
//      a fixed order (deterministic, no atomics).  Bias gradients ride along as column sums of dA.
//   3. head gradients (1- and 3-row weights): VALU reduction over point slabs.
// The chain kernels' text is frozen: the orchestration reaches them through the launcher pair below alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mi {

struct BwdArgs {
    const float* packed;     // backward stream
    const float* acts;       // saved layer inputs (regions x points)
    float* grads;            // dA regions x points (written here)
    const float* raw;        // [P,4] forward outputs (rgb post-sigmoid, sigma post-ReLU)
    const float* g_raw;      // [P,4] dL/d(raw)
    int64_t points;
    // FiLM kinds: one table [film_depth + 1][512] per group of points_per_group consecutive points
    const float* film;
    float* film_partial;     // unused by the chain (kept so the argument block stays stable)
    int64_t points_per_group, tiles_per_group, n_tiles;
    unsigned long long* stamps;   // diagnostic build (-DMI_PROFILE_STAMPS) only: [block][128] s_memtime values (MI_STAMP)
    int film_depth;          // FiLM kinds: hidden_layers (the run-time-depth chain reads it), else 0
};

// The COUNTED instances (training with an occupancy grid): the rows are the first *count entries of a device-counted list of
// point indices.  acts / grads hold COMPACT rows (row e belongs to point list[e]; a.points = the capacity, the regions'
// stride), raw / g_raw stay [all points of the pass][4] and are read at row list[e].
struct CountedBwdArgs : BwdArgs {
    const int* list;
    const int* count;
};
// rows of a counted launch (block-uniform), never more than the capacity the buffers were sized for
__device__ __forceinline__ int64_t counted_rows(const int* count, int64_t capacity) {
    const int64_t n = __builtin_amdgcn_readfirstlane(__hip_atomic_load(count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    return n < 0 ? 0 : n < capacity ? n : capacity;
}
// The slab length of the counted weight-gradient kernels: the host plans n_slabs from the CAPACITY (BwdBatcher::slabs_for /
// slab_pts_for, as for a plain pass) and sizes the partial records for it; the device cuts the rows it really has into that
// many equal slabs of whole 32-point stages, slab_len = ceil32(ceil(count / n_slabs)).  With count == capacity this is the
// host planner's slab length (n_slabs = ceil(P / slab) gives (n_slabs - 1) slab < P <= n_slabs slab, so ceil(P / n_slabs) <=
// slab, and n_slabs <= the planned slabs gives >=); n_slabs * slab_len >= count always; a slab past the rows is empty and
// writes a zero record.
__host__ __device__ constexpr int counted_slab_pts(int64_t count, int n_slabs) {
    return (int)(((count + n_slabs - 1) / n_slabs + 31) / 32 * 32);
}
struct CountedRows { const int* count; int64_t capacity; int n_slabs; };

// field_bwd_chain.hip: one chain kernel of a canonical kind (canon_kind) over `blocks` 128-point tiles - the kind's plain
// instance, or its counted one (an error for a kind that has none: the kinds no occupancy grid exists for).
int launch_bwd_chain(int kind, BwdArgs& a, unsigned blocks, hipStream_t stream);
int launch_bwd_chain_counted(int kind, CountedBwdArgs& a, unsigned blocks, hipStream_t stream);

}  // namespace mi
