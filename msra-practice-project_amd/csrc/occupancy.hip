// occupancy.hip - construction of a per-scene occupancy bit grid (gfx950): one bit per cell of a Gx x Gy x Gz grid over an
// axis-aligned box, cell (ix, iy, iz) at bit (ix Gy + iy) Gz + iz (include/mi_render.h).
//
//   occupancy_cell_points_kernel  k^3 regular sub-sample points per cell, [count k^3, 6] rows for mi_field_eval_points
//   occupancy_threshold / dilate / pack kernels   sigma at those points -> one byte per cell, dilated, packed into words
//   occupancy_mark_rays_kernel    reading a grid: the samples of a render pass that lie in occupied cells, as a device-counted list
//   occupancy_mark_ordered_kernel / occupancy_scan_blocks_kernel   the same list in ascending order, without atomics (training)
//
// Small kernels next to the field evaluations between them (cells k^3 MLP points).  Compiled with -ffp-contract=off: a
// sub-sample point is a chain of separately rounded operations, which a test restates in torch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launchers.h"
#include "mi_host.h"

namespace mi {

struct CellPointsArgs { int dims[3]; float lo[3], cell[3]; int k; };

// Row i of the output: sub-sample i % k^3 of cell head + i / k^3; sub-sample (si, sj, sk) = ((s / k) / k, (s / k) % k, s % k)
// sits at lo_c + (i_c + (s_c + 0.5) / k) * cell_c, every operation rounded on its own; direction 0 (sigma does not depend on it).
__global__ __launch_bounds__(256) void occupancy_cell_points_kernel(CellPointsArgs a, int64_t head, int64_t rows,
                                                                    float* __restrict__ pts) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    const int k3 = a.k * a.k * a.k;
    const int64_t cell = head + i / k3;
    const int s = (int)(i % k3);
    const int c[3] = {(int)(cell / ((int64_t)a.dims[1] * a.dims[2])), (int)((cell / a.dims[2]) % a.dims[1]), (int)(cell % a.dims[2])};
    const int sub[3] = {s / (a.k * a.k), (s / a.k) % a.k, s % a.k};
    float* o = pts + i * 6;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float f = __fdiv_rn(__fadd_rn((float)sub[d], 0.5f), (float)a.k);
        o[d] = __fadd_rn(a.lo[d], __fmul_rn(__fadd_rn((float)c[d], f), a.cell[d]));
        o[3 + d] = 0.f;
    }
}

int launch_occupancy_cell_points(const int* dims, const float* lo, const float* cell, int k, int64_t head, int64_t count,
                                 float* points, hipStream_t stream) {
    const int64_t rows = count * k * k * k;
    if (rows <= 0) return 0;
    if ((rows + 255) / 256 > 0x7fffffffLL) { set_error("occupancy cell points: too many rows (%lld)", (long long)rows); return -1; }
    CellPointsArgs a;
    for (int d = 0; d < 3; ++d) { a.dims[d] = dims[d]; a.lo[d] = lo[d]; a.cell[d] = cell[d]; }
    a.k = k;
    hipLaunchKernelGGL(occupancy_cell_points_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, a, head, rows, points);
    return check_launch("occupancy_cell_points");
}

// a cell is occupied iff any of its k^3 sub-samples has sigma > threshold (strict; a NaN sigma is not above anything)
__global__ __launch_bounds__(256) void occupancy_threshold_kernel(const float* __restrict__ sigma, int cells, int k3,
                                                                  float threshold, uint8_t* __restrict__ occ) {
    const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (cell >= cells) return;
    const float* s = sigma + cell * k3;
    bool any = false;
    for (int i = 0; i < k3; ++i) any = any || s[i] > threshold;
    occ[cell] = any ? 1 : 0;
}

// one step of 6-neighbourhood dilation, clipped at the box
__global__ __launch_bounds__(256) void occupancy_dilate_kernel(const uint8_t* __restrict__ in, int g0, int g1, int g2,
                                                               uint8_t* __restrict__ out) {
    const int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= (int64_t)g0 * g1 * g2) return;
    const int cell = (int)at;
    const int iz = cell % g2, iy = (cell / g2) % g1, ix = cell / (g1 * g2);
    uint8_t v = in[cell];
    if (ix > 0) v |= in[cell - g1 * g2];
    if (ix + 1 < g0) v |= in[cell + g1 * g2];
    if (iy > 0) v |= in[cell - g2];
    if (iy + 1 < g1) v |= in[cell + g2];
    if (iz > 0) v |= in[cell - 1];
    if (iz + 1 < g2) v |= in[cell + 1];
    out[cell] = v;
}

// 32 cells per thread into one word (cell index i: word i >> 5, bit i & 31); the last word's spare bits are 0
__global__ __launch_bounds__(256) void occupancy_pack_kernel(const uint8_t* __restrict__ occ, int cells, int words,
                                                             uint32_t* __restrict__ bits) {
    const int w = blockIdx.x * 256 + threadIdx.x;
    if (w >= words) return;
    uint32_t v = 0;
    for (int b = 0; b < 32; ++b) {
        const int64_t cell = (int64_t)w * 32 + b;
        if (cell < cells && occ[cell]) v |= 1u << b;
    }
    bits[w] = v;
}

// one byte per cell, a second copy for the dilation's ping-pong; each region a whole number of 256-byte blocks
static int64_t occ_region_bytes(int64_t cells) { return (cells + 255) / 256 * 256; }
int64_t occupancy_pack_workspace_bytes(int64_t cells, int dilate) { return occ_region_bytes(cells) * (dilate > 0 ? 2 : 1); }

int launch_occupancy_pack(const float* sigma, const int* dims, int k, float threshold, int dilate, uint32_t* bits,
                          void* workspace, hipStream_t stream) {
    const int cells = dims[0] * dims[1] * dims[2], words = (int)(((int64_t)cells + 31) / 32);
    uint8_t* buf[2] = {(uint8_t*)workspace, (uint8_t*)workspace + occ_region_bytes(cells)};
    const dim3 grid((unsigned)(((int64_t)cells + 255) / 256));
    hipLaunchKernelGGL(occupancy_threshold_kernel, grid, dim3(256), 0, stream, sigma, cells, k * k * k, threshold, buf[0]);
    if (const int rc = check_launch("occupancy_threshold")) return rc;
    int cur = 0;
    for (int i = 0; i < dilate; ++i, cur ^= 1) {
        hipLaunchKernelGGL(occupancy_dilate_kernel, grid, dim3(256), 0, stream, buf[cur], dims[0], dims[1], dims[2], buf[cur ^ 1]);
        if (const int rc = check_launch("occupancy_dilate")) return rc;
    }
    hipLaunchKernelGGL(occupancy_pack_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, stream, buf[cur], cells, words, bits);
    return check_launch("occupancy_pack");
}

// ---- reading a grid: which samples of a pass are evaluated (mi_occupancy_mark_rays; MarkArgs: launchers.h) -----------------------
// The rule every layer of rendering with a grid is tested against.  The point is the one the fused forward evaluates
// (field_mlp_device.h: load_point, p = o + d z, a multiply and an add), placed by t = (p - lo) * inv_cell (a subtract and a
// multiply); inside iff 0 <= t < G on every axis, so a NaN is not inside; its cell is floor(t).
__device__ __forceinline__ bool point_occupied(const MarkArgs& g, const uint32_t* __restrict__ bits, const float* __restrict__ rays,
                                               const float* __restrict__ z, int64_t p, int S) {
    const float* r = rays + (p / S) * 6;
    const float zz = z[p];
    float t[3];
    bool inside = true;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float x = __fadd_rn(r[d], __fmul_rn(r[3 + d], zz));
        t[d] = __fmul_rn(__fsub_rn(x, g.lo[d]), g.inv_cell[d]);
        inside = inside && t[d] >= 0.f && t[d] < (float)g.dims[d];
    }
    if (!inside) return false;
    const int bit = ((int)floorf(t[0]) * g.dims[1] + (int)floorf(t[1])) * g.dims[2] + (int)floorf(t[2]);
    return (bits[bit >> 5] >> (bit & 31)) & 1u;
}

// One thread per point, kMarkPerThread rounds of 256 points per workgroup.  A frame's 10^8 points must not queue on the one
// counter wave by wave, so a workgroup compacts its 4096 points itself: every round's ballot gives a per-wave count in LDS,
// one thread turns the 64 counts into exclusive offsets and takes ONE atomic for the workgroup's slots, and a point's slot is
// the workgroup's base + its (round, wave) offset + the occupied lanes below it.  Unoccupied points get their raw row zeroed
// (a vector store); occupied rows are not touched.  The list has room for every point, so it cannot overflow.
constexpr int kMarkPerThread = 16;
constexpr int kMarkBlock = 256 * kMarkPerThread;

__global__ __launch_bounds__(256) void occupancy_mark_rays_kernel(MarkArgs g, const uint32_t* __restrict__ bits,
                                                                  const float* __restrict__ rays, const float* __restrict__ z,
                                                                  int64_t total, int S, int* __restrict__ list, int* count,
                                                                  float* __restrict__ raw) {
    __shared__ int offs[kMarkPerThread * 4];
    __shared__ int base_s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t p0 = (int64_t)blockIdx.x * kMarkBlock + threadIdx.x;
    uint32_t mine = 0;                                          // bit `it`: this thread's point of round `it` is occupied
    for (int it = 0; it < kMarkPerThread; ++it) {
        const int64_t p = p0 + it * 256;
        bool occ = false;
        if (p < total) {
            occ = point_occupied(g, bits, rays, z, p, S);
            if (!occ && raw) reinterpret_cast<float4*>(raw)[p] = float4{0.f, 0.f, 0.f, 0.f};
        }
        const uint64_t b = __ballot(occ);
        if (lane == 0) offs[it * 4 + wave] = __popcll(b);
        mine |= (uint32_t)occ << it;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int sum = 0;
        for (int i = 0; i < kMarkPerThread * 4; ++i) { const int c = offs[i]; offs[i] = sum; sum += c; }
        base_s = sum ? __hip_atomic_fetch_add(count, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
    }
    __syncthreads();
    const int base = base_s;
    for (int it = 0; it < kMarkPerThread; ++it) {
        const bool occ = (mine >> it) & 1u;
        const uint64_t b = __ballot(occ);
        if (occ) list[base + offs[it * 4 + wave] + __popcll(b & ((1ull << lane) - 1))] = (int)(p0 + it * 256);
    }
}

int launch_occupancy_mark_rays(const OccupancyGridArgs& grid, const float* rays, const float* z, int64_t n, int S, int* list,
                               int* count, float* raw, hipStream_t stream) {
    if (hipMemsetAsync(count, 0, sizeof(int), stream) != hipSuccess) { set_error("occupancy mark: hipMemsetAsync failed"); return -2; }
    const int64_t total = n * S;
    if (total <= 0) return 0;
    hipLaunchKernelGGL(occupancy_mark_rays_kernel, dim3((unsigned)((total + kMarkBlock - 1) / kMarkBlock)), dim3(256), 0, stream,
                       grid.cells, grid.bits, rays, z, total, S, list, count, raw);
    return check_launch("occupancy_mark_rays");
}

// ---- the same list in ascending order, without atomics (mi_occupancy_mark_rays_ordered: training with a grid) --------------------
// The list order is the row order of the weight-gradient sums, so it must not depend on which workgroup's atomic lands first.
// Inside a workgroup the kernel above already writes ascending indices ((round, wave, lane) order IS point order); only the
// workgroups' bases are timing-dependent.  Three launches replace the atomic:
//   count   : the occupancy test, the zeroing of unlisted raw rows, one count per workgroup into blk[workgroup];
//   scan    : one workgroup turns blk[] into exclusive offsets and writes their total to the device count;
//   scatter : the occupancy test again (a few loads per point: cheaper than keeping 4096 bits per workgroup in memory), slots
//             from blk[workgroup] + the (round, wave) offset + the occupied lanes below.
// blk lies behind the list's n * S entries: one int per workgroup of kMarkBlock points (occupancy_ordered_list_ints).
template <bool SCATTER>
__global__ __launch_bounds__(256) void occupancy_mark_ordered_kernel(MarkArgs g, const uint32_t* __restrict__ bits,
                                                                     const float* __restrict__ rays, const float* __restrict__ z,
                                                                     int64_t total, int S, int* __restrict__ list, int* __restrict__ blk,
                                                                     float* __restrict__ raw) {
    __shared__ int offs[kMarkPerThread * 4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t p0 = (int64_t)blockIdx.x * kMarkBlock + threadIdx.x;
    uint32_t mine = 0;                                          // bit `it`: this thread's point of round `it` is occupied
    for (int it = 0; it < kMarkPerThread; ++it) {
        const int64_t p = p0 + it * 256;
        bool occ = false;
        if (p < total) {
            occ = point_occupied(g, bits, rays, z, p, S);
            if (!SCATTER && !occ && raw) reinterpret_cast<float4*>(raw)[p] = float4{0.f, 0.f, 0.f, 0.f};
        }
        const uint64_t b = __ballot(occ);
        if (lane == 0) offs[it * 4 + wave] = __popcll(b);
        mine |= (uint32_t)occ << it;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int sum = 0;
        for (int i = 0; i < kMarkPerThread * 4; ++i) { const int c = offs[i]; offs[i] = sum; sum += c; }
        if (!SCATTER) blk[blockIdx.x] = sum;
    }
    if (!SCATTER) return;
    __syncthreads();
    const int base = blk[blockIdx.x];
    for (int it = 0; it < kMarkPerThread; ++it) {
        const bool occ = (mine >> it) & 1u;
        const uint64_t b = __ballot(occ);
        if (occ) list[base + offs[it * 4 + wave] + __popcll(b & ((1ull << lane) - 1))] = (int)(p0 + it * 256);
    }
}

// blk[0 .. n_blocks) -> its exclusive prefix sums, their total -> *count.  One workgroup: thread t sums a run of consecutive
// entries, thread 0 scans the 256 run sums, every thread rewrites its run (a frame's 30 000 entries are 118 per thread).
__global__ __launch_bounds__(256) void occupancy_scan_blocks_kernel(int* __restrict__ blk, int n_blocks, int* __restrict__ count) {
    __shared__ int part[256];
    const int per = (n_blocks + 255) / 256, t = threadIdx.x;
    const int lo = t * per < n_blocks ? t * per : n_blocks, hi = lo + per < n_blocks ? lo + per : n_blocks;
    int s = 0;
    for (int i = lo; i < hi; ++i) s += blk[i];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        int sum = 0;
        for (int i = 0; i < 256; ++i) { const int c = part[i]; part[i] = sum; sum += c; }
        *count = sum;
    }
    __syncthreads();
    int run = part[t];
    for (int i = lo; i < hi; ++i) { const int c = blk[i]; blk[i] = run; run += c; }
}

int64_t occupancy_ordered_list_ints(int64_t points) { return points + (points + kMarkBlock - 1) / kMarkBlock; }

int launch_occupancy_mark_rays_ordered(const OccupancyGridArgs& grid, const float* rays, const float* z, int64_t n, int S, int* list,
                                       int* count, float* raw, hipStream_t stream) {
    const int64_t total = n * S;
    if (total <= 0) {
        if (hipMemsetAsync(count, 0, sizeof(int), stream) != hipSuccess) { set_error("occupancy mark: hipMemsetAsync failed"); return -2; }
        return 0;
    }
    const int n_blocks = (int)((total + kMarkBlock - 1) / kMarkBlock);
    int* blk = list + total;
    hipLaunchKernelGGL(occupancy_mark_ordered_kernel<false>, dim3((unsigned)n_blocks), dim3(256), 0, stream, grid.cells, grid.bits, rays, z,
                       total, S, list, blk, raw);
    if (const int rc = check_launch("occupancy_mark_ordered (count)")) return rc;
    hipLaunchKernelGGL(occupancy_scan_blocks_kernel, dim3(1), dim3(256), 0, stream, blk, n_blocks, count);
    if (const int rc = check_launch("occupancy_scan_blocks")) return rc;
    hipLaunchKernelGGL(occupancy_mark_ordered_kernel<true>, dim3((unsigned)n_blocks), dim3(256), 0, stream, grid.cells, grid.bits, rays, z,
                       total, S, list, blk, raw);
    return check_launch("occupancy_mark_ordered (scatter)");
}

}  // namespace mi
