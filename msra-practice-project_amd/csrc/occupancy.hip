// occupancy.hip - construction of a per-scene occupancy bit grid (gfx950): one bit per cell of a Gx x Gy x Gz grid over an
// axis-aligned box, cell (ix, iy, iz) at bit (ix Gy + iy) Gz + iz (include/mi_render.h).
//
//   occupancy_cell_points_kernel  k^3 regular sub-sample points per cell, [count k^3, 6] rows for mi_field_eval_points
//   occupancy_threshold / dilate / pack kernels   sigma at those points -> one byte per cell, dilated, packed into words
//   occupancy_draw_points_kernel / occupancy_density_* kernels   a live grid: one jittered point in each of a drawn subset of
//                                 the cells, the decayed-maximum fold of their sigma into a per-cell density, its re-thresholding
//   occupancy_mark_rays_kernel    reading a grid: the samples of a render pass that lie in occupied cells, as a device-counted list
//   occupancy_mark_ordered_kernel / occupancy_scan_blocks_kernel   the same list in ascending order, without atomics (training)
//   occupancy_clip_rays_kernel    reading a grid: each ray's sampling range clipped to the first and last occupied probe along it
//
// Small kernels next to the field evaluations between them (cells k^3 MLP points).  Compiled with -ffp-contract=off: a
// sub-sample point is a chain of separately rounded operations, which a test restates in torch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launchers.h"
#include "mi_host.h"
#include "mi_philox.h"

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

// the byte plane buf[0] dilated `dilate` times (ping-pong with buf[1]) and packed into words: the end of both packs
static int dilate_and_pack(uint8_t* const buf[2], const int* dims, int dilate, uint32_t* bits, hipStream_t stream) {
    const int cells = dims[0] * dims[1] * dims[2], words = (int)(((int64_t)cells + 31) / 32);
    const dim3 grid((unsigned)(((int64_t)cells + 255) / 256));
    int cur = 0;
    for (int i = 0; i < dilate; ++i, cur ^= 1) {
        hipLaunchKernelGGL(occupancy_dilate_kernel, grid, dim3(256), 0, stream, buf[cur], dims[0], dims[1], dims[2], buf[cur ^ 1]);
        if (const int rc = check_launch("occupancy_dilate")) return rc;
    }
    hipLaunchKernelGGL(occupancy_pack_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, stream, buf[cur], cells, words, bits);
    return check_launch("occupancy_pack");
}

int launch_occupancy_pack(const float* sigma, const int* dims, int k, float threshold, int dilate, uint32_t* bits,
                          void* workspace, hipStream_t stream) {
    const int cells = dims[0] * dims[1] * dims[2];
    uint8_t* buf[2] = {(uint8_t*)workspace, (uint8_t*)workspace + occ_region_bytes(cells)};
    hipLaunchKernelGGL(occupancy_threshold_kernel, dim3((unsigned)(((int64_t)cells + 255) / 256)), dim3(256), 0, stream, sigma, cells,
                       k * k * k, threshold, buf[0]);
    if (const int rc = check_launch("occupancy_threshold")) return rc;
    return dilate_and_pack(buf, dims, dilate, bits, stream);
}

// ---- a live grid: jittered partial re-sampling of a per-cell density, folded by a decayed maximum (include/mi_render.h) ---------
// Row r of update `epoch` reads the words of Philox stream (epoch << 32) | r: words 0..2 are the jitter inside its cell,
// word 3 is the cell of a uniformly drawn row, words 4..11 are the candidates of a row drawn among the occupied cells (the
// first one whose bit is set, the last one if none is: rejection, so no compaction and no atomic).
struct DrawArgs { int dims[3]; float lo[3], cell[3]; };

__global__ __launch_bounds__(256) void occupancy_draw_points_kernel(DrawArgs a, const uint32_t* __restrict__ bits, uint32_t cells,
                                                                    uint64_t seed, uint32_t epoch, int mode, int64_t row0,
                                                                    int64_t count, int64_t n_uniform, int* __restrict__ cell_ids,
                                                                    float* __restrict__ pts) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int64_t r = row0 + i;
    const uint64_t stream = ((uint64_t)epoch << 32) | (uint64_t)r;
    uint32_t cell = 0;
    if (mode == 0) {
        cell = (uint32_t)r;
    } else if (r < n_uniform) {
        cell = (uint32_t)(((uint64_t)philox_u32(seed, stream, 3) * cells) >> 32);
    } else {
        for (uint32_t t = 0; t < 8; ++t) {
            cell = (uint32_t)(((uint64_t)philox_u32(seed, stream, 4 + t) * cells) >> 32);
            if ((bits[cell >> 5] >> (cell & 31)) & 1u) break;
        }
    }
    const uint32_t plane = (uint32_t)a.dims[1] * (uint32_t)a.dims[2];
    const uint32_t c[3] = {cell / plane, (cell / (uint32_t)a.dims[2]) % (uint32_t)a.dims[1], cell % (uint32_t)a.dims[2]};
    cell_ids[i] = (int)cell;
    float* o = pts + i * 6;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float u = (float)(philox_u32(seed, stream, (uint32_t)d) >> 8) * 0x1p-24f;
        o[d] = __fadd_rn(a.lo[d], __fmul_rn(__fadd_rn((float)c[d], u), a.cell[d]));
        o[3 + d] = 0.f;
    }
}

int launch_occupancy_draw_points(const uint32_t* bits, const int* dims, const float* lo, const float* cell, uint64_t seed,
                                 uint32_t epoch, int mode, int64_t row0, int64_t count, int64_t n_uniform, int* cell_ids,
                                 float* points, hipStream_t stream) {
    if (count <= 0) return 0;
    DrawArgs a;
    for (int d = 0; d < 3; ++d) { a.dims[d] = dims[d]; a.lo[d] = lo[d]; a.cell[d] = cell[d]; }
    const uint32_t cells = (uint32_t)(dims[0] * dims[1] * dims[2]);
    hipLaunchKernelGGL(occupancy_draw_points_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, a, bits, cells, seed,
                       epoch, mode, row0, count, n_uniform, cell_ids, points);
    return check_launch("occupancy_draw_points");
}

// The fold of one update: density_c = max(density_c * decay, the largest sigma sampled in cell c), cells without a sample
// untouched.  Three kernels: the scratch ints are set to -1 ("unsampled"); every row takes an integer atomicMax of the bits of
// max(sigma, +0) - for non-negative floats the integer order is the float order, so the result does not depend on the order of
// arrival, and +0 (bits 0) lies above the sentinel where -0.0 (bits 0x80000000, a negative int) would lie below it; then one
// thread per cell folds.  A row whose cell id is outside the grid is ignored.
__global__ __launch_bounds__(256) void occupancy_density_clear_kernel(int cells, int* __restrict__ scratch) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c < cells) scratch[c] = -1;
}

__global__ __launch_bounds__(256) void occupancy_density_max_kernel(const float* __restrict__ sigma, const int* __restrict__ cell_ids,
                                                                    int64_t count, int cells, int* scratch) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int c = cell_ids[i];
    if (c < 0 || c >= cells) return;
    const float s = sigma[i];
    const float v = s > 0.f ? s : 0.f;                          // -0.0, negatives and NaN: +0
    atomicMax(scratch + c, __float_as_int(v));
}

__global__ __launch_bounds__(256) void occupancy_density_fold_kernel(const int* __restrict__ scratch, int cells, float decay,
                                                                     float* __restrict__ density) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= cells) return;
    const int m = scratch[c];
    if (m < 0) return;
    density[c] = fmaxf(__fmul_rn(density[c], decay), __int_as_float(m));
}

// The workspace of the density calls: the scratch ints of the fold; the fp64 partial sums of the pack, one per workgroup of
// kSumBlock cells; the pack's mean and threshold (two floats); the byte planes of occupancy_pack_workspace_bytes.
constexpr int kSumBlock = 4096;
static int64_t round256(int64_t bytes) { return (bytes + 255) / 256 * 256; }
static int64_t density_sum_blocks(int64_t cells) { return (cells + kSumBlock - 1) / kSumBlock; }
static int64_t density_scratch_bytes(int64_t cells) { return round256(cells * 4); }
static int64_t density_partial_bytes(int64_t cells) { return round256(density_sum_blocks(cells) * 8); }
int64_t occupancy_density_workspace_bytes(int64_t cells, int dilate) {
    return density_scratch_bytes(cells) + density_partial_bytes(cells) + 256 + occupancy_pack_workspace_bytes(cells, dilate);
}

int launch_occupancy_density_update(const float* sigma, const int* cell_ids, int64_t count, const int* dims, float decay,
                                    float* density, void* workspace, hipStream_t stream) {
    if (count <= 0) return 0;
    const int cells = dims[0] * dims[1] * dims[2];
    int* scratch = (int*)workspace;
    const dim3 grid((unsigned)(((int64_t)cells + 255) / 256));
    hipLaunchKernelGGL(occupancy_density_clear_kernel, grid, dim3(256), 0, stream, cells, scratch);
    if (const int rc = check_launch("occupancy_density_clear")) return rc;
    hipLaunchKernelGGL(occupancy_density_max_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, sigma, cell_ids, count,
                       cells, scratch);
    if (const int rc = check_launch("occupancy_density_max")) return rc;
    hipLaunchKernelGGL(occupancy_density_fold_kernel, grid, dim3(256), 0, stream, scratch, cells, decay, density);
    return check_launch("occupancy_density_fold");
}

// The mean of the density in fp64, in a fixed order so that two runs give the same bits: thread t of a workgroup adds its 16
// cells (t, t + 256, ...) in ascending order, the 256 sums are halved in LDS (a fixed tree), and one workgroup then adds the
// workgroups' sums in index order.  No float atomics.
__global__ __launch_bounds__(256) void occupancy_density_sum_kernel(const float* __restrict__ density, int cells,
                                                                    double* __restrict__ partial) {
    __shared__ double part[256];
    const int64_t base = (int64_t)blockIdx.x * kSumBlock + threadIdx.x;
    double s = 0.0;
    for (int it = 0; it < kSumBlock / 256; ++it) {
        const int64_t c = base + it * 256;
        if (c < cells) s += (double)density[c];
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) part[threadIdx.x] += part[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = part[0];
}

// out[0] = mean = float(sum / cells), out[1] = thr = relative ? fminf(threshold, mean) : threshold
__global__ __launch_bounds__(256) void occupancy_density_mean_kernel(const double* __restrict__ partial, int n_blocks, int cells,
                                                                     float threshold, int relative, float* __restrict__ out) {
    __shared__ double part[256];
    double sum = 0.0;
    for (int head = 0; head < n_blocks; head += 256) {
        const int i = head + (int)threadIdx.x;
        part[threadIdx.x] = i < n_blocks ? partial[i] : 0.0;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int n = n_blocks - head < 256 ? n_blocks - head : 256;
            for (int j = 0; j < n; ++j) sum += part[j];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float mean = (float)(sum / (double)cells);
        out[0] = mean;
        out[1] = relative ? fminf(threshold, mean) : threshold;
    }
}

// a cell is occupied iff its density is above the device threshold (strict)
__global__ __launch_bounds__(256) void occupancy_density_threshold_kernel(const float* __restrict__ density, int cells,
                                                                          const float* __restrict__ mean_thr,
                                                                          uint8_t* __restrict__ occ) {
    const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (cell >= cells) return;
    occ[cell] = density[cell] > mean_thr[1] ? 1 : 0;
}

int launch_occupancy_density_pack(const float* density, const int* dims, float threshold, int relative, int dilate, uint32_t* bits,
                                  void* workspace, hipStream_t stream) {
    const int cells = dims[0] * dims[1] * dims[2];
    const int n_blocks = (int)density_sum_blocks(cells);
    uint8_t* at = (uint8_t*)workspace + density_scratch_bytes(cells);
    double* partial = (double*)at;
    float* mean_thr = (float*)(at + density_partial_bytes(cells));
    uint8_t* planes = at + density_partial_bytes(cells) + 256;
    uint8_t* buf[2] = {planes, planes + occ_region_bytes(cells)};
    hipLaunchKernelGGL(occupancy_density_sum_kernel, dim3((unsigned)n_blocks), dim3(256), 0, stream, density, cells, partial);
    if (const int rc = check_launch("occupancy_density_sum")) return rc;
    hipLaunchKernelGGL(occupancy_density_mean_kernel, dim3(1), dim3(256), 0, stream, partial, n_blocks, cells, threshold, relative,
                       mean_thr);
    if (const int rc = check_launch("occupancy_density_mean")) return rc;
    hipLaunchKernelGGL(occupancy_density_threshold_kernel, dim3((unsigned)(((int64_t)cells + 255) / 256)), dim3(256), 0, stream, density,
                       cells, mean_thr, buf[0]);
    if (const int rc = check_launch("occupancy_density_threshold")) return rc;
    return dilate_and_pack(buf, dims, dilate, bits, stream);
}

// ---- reading a grid: which samples of a pass are evaluated (mi_occupancy_mark_rays; MarkArgs: launchers.h) -----------------------
// The rule every layer of rendering with a grid is tested against.  The point is the one the fused forward evaluates
// (field_mlp_device.h: load_point, p = o + d z, a multiply and an add), placed by t = (p - lo) * inv_cell (a subtract and a
// multiply); inside iff 0 <= t < G on every axis, so a NaN is not inside; its cell is floor(t).
// ... of the ray r (its six floats) at depth zz: the test itself, which the mark kernels and the clip kernel share
__device__ __forceinline__ bool depth_occupied(const MarkArgs& g, const uint32_t* __restrict__ bits, const float* __restrict__ r,
                                               float zz) {
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

// point p = ray * S + k of a pass over rays [n,2,3] at depths z [n,S]
__device__ __forceinline__ bool point_occupied(const MarkArgs& g, const uint32_t* __restrict__ bits, const float* __restrict__ rays,
                                               const float* __restrict__ z, int64_t p, int S) {
    return depth_occupied(g, bits, rays + (p / S) * 6, z[p]);
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

// ---- clipping a ray's sampling range to the grid (mi_occupancy_clip_rays) ---------------------------------------------------------
// The rule: M probes at the midpoints of M equal bins of [near, far], h = (far - near) / float(M), t_k = near + (float(k) + 0.5f) * h,
// each tested by depth_occupied like a sample of a pass.  With k0 / k1 the least / greatest occupied probe, a = max(k0 - pad, 0),
// b = min(k1 + 1 + pad, M): near_r = near + float(a) * h, far_r = far itself where b == M, else near + float(b) * h.  A ray
// without an occupied probe keeps (near, far): the mark culls its samples as it does without clipping.
// One wave per ray, four rays per workgroup, the grid strided over the rays.  Lane l of round j tests probe 64 j + l and the
// round's ballot is its mask: rounds run from the front until the first non-zero mask (k0 = its lowest bit), then from the back
// down to that round (k1 = the highest bit of the first non-zero mask met), so a ray that is occupied near both ends of its
// range reads two rounds.  Every branch is on a ballot or on the ray index: uniform over the wave.  Lanes 0 and 1 store the
// two floats; no LDS, no atomics.
__global__ __launch_bounds__(256) void occupancy_clip_rays_kernel(MarkArgs g, const uint32_t* __restrict__ bits,
                                                                  const float* __restrict__ rays, int64_t n, float near_, float far_,
                                                                  int probes, int pad, float* __restrict__ bounds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float h = __fdiv_rn(__fsub_rn(far_, near_), (float)probes);
    const int rounds = (probes + 63) >> 6;
    for (int64_t ray = (int64_t)blockIdx.x * 4 + wave; ray < n; ray += (int64_t)gridDim.x * 4) {
        const float* r = rays + ray * 6;
        const auto round_mask = [&](int j) {
            const int k = j * 64 + lane;
            const float t = __fadd_rn(near_, __fmul_rn(__fadd_rn((float)k, 0.5f), h));
            return __builtin_amdgcn_ballot_w64(k < probes && depth_occupied(g, bits, r, t));
        };
        int k0 = -1, k1 = -1, j0 = 0;
        uint64_t first = 0;
        for (; j0 < rounds; ++j0)
            if ((first = round_mask(j0)) != 0ull) { k0 = j0 * 64 + __builtin_ctzll(first); break; }
        for (int j = rounds - 1; k0 >= 0 && j >= j0; --j) {
            const uint64_t m = j == j0 ? first : round_mask(j);
            if (m != 0ull) { k1 = j * 64 + 63 - __builtin_clzll(m); break; }
        }
        float lo_r = near_, hi_r = far_;
        if (k0 >= 0) {
            const int a = k0 - pad > 0 ? k0 - pad : 0;
            const int b = k1 + 1 + pad < probes ? k1 + 1 + pad : probes;
            lo_r = __fadd_rn(near_, __fmul_rn((float)a, h));
            if (b != probes) hi_r = __fadd_rn(near_, __fmul_rn((float)b, h));
        }
        if (lane < 2) bounds[ray * 2 + lane] = lane ? hi_r : lo_r;
    }
}

int launch_occupancy_clip_rays(const OccupancyGridArgs& grid, const float* rays, int64_t n, float near_, float far_, int probes,
                               int pad, float* bounds, hipStream_t stream) {
    if (n <= 0) return 0;
    int64_t blocks = (n + 3) / 4;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(occupancy_clip_rays_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, grid.cells, grid.bits, rays, n, near_,
                       far_, probes, pad, bounds);
    return check_launch("occupancy_clip_rays");
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
