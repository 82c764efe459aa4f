// mesh_stages.hip - marching cubes on the device: the mesh half of create_mesh (pi_GAN/utils.py:109-180,
// skimage.measure.marching_cubes_lewiner with allow_degenerate=True).
//
//   mc_count_kernel      per-block vertex / triangle totals + the volume's min / max   one volume sweep
//   scan_block_kernel    exclusive scan of int64 block totals (1024 per block)          hand-written two-level scan
//   scan_add_kernel      adds the scanned block sums back
//   mc_verts_kernel      vertices (position, normal, value) + a 16-bit tag per corner   one volume sweep
//   mc_faces_kernel      triangles, vertex ids from the tags                            one volume sweep
//
// Thread = volume corner (C order over [X, Y, Z], Z fastest).  A corner owns the edges that leave it along +x, +y,
// +z and, when it is a cube's low corner, that cube.  Vertices are numbered by owning corner, then axis; triangles by
// cube (linear index of its low corner), then loop, then fan position (mesh_cube.h).  Output offsets come from
// count -> exclusive scan -> emit, so the result is the same bit for bit on every run (no atomics order anything;
// the only atomics are the min / max of the range check, which are order-independent).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mi_render.h"
#include "launchers.h"
#include "mesh_cube.h"
#include "mi_host.h"

namespace mi {

constexpr int kMcBlock = 256;          // corners per workgroup of the three sweeps
constexpr int kScanItems = 4;
constexpr int kScanSpan = kMcBlock * kScanItems;   // int64 entries per scan workgroup

struct McVol {
    const float* v;
    int64_t nx, ny, nz;
    double level;
    __device__ __forceinline__ float at(int64_t x, int64_t y, int64_t z) const { return v[(x * ny + y) * nz + z]; }
};

// bits 0..2: which of the corner's +x / +y / +z edges cross the level
__device__ __forceinline__ int edge_mask(const McVol& m, int64_t x, int64_t y, int64_t z) {
    const bool in0 = (double)m.at(x, y, z) > m.level;
    int mask = 0;
    if (x + 1 < m.nx && (((double)m.at(x + 1, y, z) > m.level) != in0)) mask |= 1;
    if (y + 1 < m.ny && (((double)m.at(x, y + 1, z) > m.level) != in0)) mask |= 2;
    if (z + 1 < m.nz && (((double)m.at(x, y, z + 1) > m.level) != in0)) mask |= 4;
    return mask;
}

__device__ __forceinline__ bool is_cube(const McVol& m, int64_t x, int64_t y, int64_t z) {
    return x + 1 < m.nx && y + 1 < m.ny && z + 1 < m.nz;
}

__device__ __forceinline__ int cube_tris(const McVol& m, int64_t x, int64_t y, int64_t z, mc::Loops& L) {
    double a[8];
    for (int b = 0; b < 8; ++b) a[b] = (double)m.at(x + ((b >> 2) & 1), y + ((b >> 1) & 1), z + (b & 1)) - m.level;
    return mc::cube_loops(a, L);
}

// float -> int with the same order (no NaN): atomicMin / atomicMax on ints
__device__ __forceinline__ int ordered(float f) {
    const int i = __float_as_int(f);
    return i >= 0 ? i : i ^ 0x7fffffff;
}

// block-wide exclusive scan of one int per thread (Hillis-Steele in LDS); returns the block total in *total
__device__ __forceinline__ int block_excl_scan(int x, int* lds, int* total) {
    const int t = threadIdx.x;
    lds[t] = x;
    __syncthreads();
    for (int d = 1; d < kMcBlock; d <<= 1) {
        const int y = t >= d ? lds[t - d] : 0;
        __syncthreads();
        lds[t] += y;
        __syncthreads();
    }
    const int incl = lds[t];
    *total = lds[kMcBlock - 1];
    __syncthreads();
    return incl - x;
}

__global__ __launch_bounds__(kMcBlock) void mc_count_kernel(McVol m, int64_t n, int64_t* __restrict__ block_v,
                                                            int64_t* __restrict__ block_f, int* __restrict__ minmax) {
    __shared__ int lds[kMcBlock];
    const int64_t i = (int64_t)blockIdx.x * kMcBlock + threadIdx.x;
    int nv = 0, nf = 0;
    float v = 0.f;
    if (i < n) {
        const int64_t z = i % m.nz, y = (i / m.nz) % m.ny, x = i / (m.nz * m.ny);
        v = m.v[i];
        nv = __popc(edge_mask(m, x, y, z));
        if (is_cube(m, x, y, z)) {
            mc::Loops L;
            nf = cube_tris(m, x, y, z, L);
        }
    }
    int tv, tf;
    block_excl_scan(nv, lds, &tv);
    block_excl_scan(nf, lds, &tf);
    // min / max of the volume (the level check): wave-reduce, one atomic per wave
    int lo = i < n ? ordered(v) : INT32_MAX, hi = i < n ? ordered(v) : INT32_MIN;
    for (int off = 32; off > 0; off >>= 1) {
        lo = min(lo, __shfl_xor(lo, off));
        hi = max(hi, __shfl_xor(hi, off));
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMin(&minmax[0], lo);
        atomicMax(&minmax[1], hi);
    }
    if (threadIdx.x == 0) {
        block_v[blockIdx.x] = tv;
        block_f[blockIdx.x] = tf;
    }
}

__global__ void minmax_init_kernel(int* minmax) {
    minmax[0] = INT32_MAX;
    minmax[1] = INT32_MIN;
}

// exclusive scan of data[0, n) in place, kScanSpan entries per workgroup; the workgroup's total goes to sums[block]
__global__ __launch_bounds__(kMcBlock) void scan_block_kernel(int64_t* __restrict__ data, int64_t n,
                                                              int64_t* __restrict__ sums) {
    __shared__ int64_t lds[kMcBlock];
    const int t = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * kScanSpan + (int64_t)t * kScanItems;
    int64_t x[kScanItems], run = 0;
    for (int k = 0; k < kScanItems; ++k) {
        x[k] = base + k < n ? data[base + k] : 0;
        run += x[k];
    }
    lds[t] = run;
    __syncthreads();
    for (int d = 1; d < kMcBlock; d <<= 1) {
        const int64_t y = t >= d ? lds[t - d] : 0;
        __syncthreads();
        lds[t] += y;
        __syncthreads();
    }
    int64_t acc = lds[t] - run;
    for (int k = 0; k < kScanItems; ++k) {
        if (base + k < n) data[base + k] = acc;
        acc += x[k];
    }
    if (t == kMcBlock - 1) sums[blockIdx.x] = lds[t];
}

__global__ __launch_bounds__(kMcBlock) void scan_add_kernel(int64_t* __restrict__ data, int64_t n,
                                                            const int64_t* __restrict__ offs) {
    const int64_t i = (int64_t)blockIdx.x * kScanSpan + threadIdx.x;
    const int64_t o = offs[blockIdx.x];
    for (int k = 0; k < kScanItems; ++k)
        if (i + k * kMcBlock < n) data[i + k * kMcBlock] += o;
}

static int64_t div_up(int64_t a, int64_t b) { return (a + b - 1) / b; }

// int64 entries of scan scratch that scan_excl(n) needs
static int64_t scan_scratch(int64_t n) {
    const int64_t nb = div_up(n, kScanSpan);
    return nb <= 1 ? 1 : nb + scan_scratch(nb);
}

static int scan_excl(int64_t* data, int64_t n, int64_t* scratch, hipStream_t s) {
    const int64_t nb = div_up(n, kScanSpan);
    hipLaunchKernelGGL(scan_block_kernel, dim3((unsigned)nb), dim3(kMcBlock), 0, s, data, n, scratch);
    if (nb > 1) {
        if (int rc = scan_excl(scratch, nb, scratch + nb, s)) return rc;
        hipLaunchKernelGGL(scan_add_kernel, dim3((unsigned)nb), dim3(kMcBlock), 0, s, data, n, scratch);
    }
    return check_launch("marching cubes scan");
}

// np.gradient of the volume at a corner along axis k: central inside, one-sided at the border
__device__ __forceinline__ double grad_axis(const McVol& m, int64_t c[3], int k) {
    const int64_t dim = k == 0 ? m.nx : k == 1 ? m.ny : m.nz;
    int64_t lo[3] = {c[0], c[1], c[2]}, hi[3] = {c[0], c[1], c[2]};
    double h = 0.5;
    if (c[k] == 0) { hi[k] = 1; h = 1.0; }
    else if (c[k] == dim - 1) { lo[k] = dim - 2; h = 1.0; }
    else { lo[k] = c[k] - 1; hi[k] = c[k] + 1; }
    return ((double)m.at(hi[0], hi[1], hi[2]) - (double)m.at(lo[0], lo[1], lo[2])) * h;
}

// Vertex tag of a corner: (index of its first vertex within its workgroup) << 3 | edge mask.  A workgroup of 256
// corners owns at most 768 vertices, so the tag fits 16 bits.
__global__ __launch_bounds__(kMcBlock) void mc_verts_kernel(McVol m, int64_t n, const int64_t* __restrict__ block_v,
                                                            double sx, double sy, double sz,
                                                            float* __restrict__ verts, float* __restrict__ normals,
                                                            float* __restrict__ values, uint16_t* __restrict__ tag) {
    __shared__ int lds[kMcBlock];
    const int64_t i = (int64_t)blockIdx.x * kMcBlock + threadIdx.x;
    int64_t c[3] = {0, 0, 0};
    int mask = 0;
    if (i < n) {
        c[2] = i % m.nz; c[1] = (i / m.nz) % m.ny; c[0] = i / (m.nz * m.ny);
        mask = edge_mask(m, c[0], c[1], c[2]);
    }
    int total;
    const int local = block_excl_scan(__popc(mask), lds, &total);
    if (i >= n) return;
    tag[i] = (uint16_t)((local << 3) | mask);
    int64_t out = block_v[blockIdx.x] + local;
    const double sp[3] = {sx, sy, sz};
    for (int a = 0; a < 3; ++a) {
        if (!((mask >> a) & 1)) continue;
        int64_t c1[3] = {c[0], c[1], c[2]};
        c1[a] += 1;
        const double a0 = (double)m.at(c[0], c[1], c[2]) - m.level, a1 = (double)m.at(c1[0], c1[1], c1[2]) - m.level;
        const double t = -a0 / (a1 - a0);
        float* p = verts + out * 3;
        for (int k = 0; k < 3; ++k) {
            const float q = (float)((double)c[k] + (k == a ? t : 0.0));
            p[k] = sp[k] == 1.0 ? q : (float)((double)q * sp[k]);
        }
        // normal: the gradient interpolated along the edge, normalised, pointing toward lower values
        double g[3], nn = 0.0;
        for (int k = 0; k < 3; ++k) {
            const double g0 = grad_axis(m, c, k), g1 = grad_axis(m, c1, k);
            g[k] = g0 + t * (g1 - g0);
            nn += g[k] * g[k];
        }
        const double inv = nn > 0.0 ? -1.0 / sqrt(nn) : 0.0;
        for (int k = 0; k < 3; ++k) normals[out * 3 + k] = (float)(g[k] * inv);
        // value: max - min of the first cube (C order) that holds the edge
        int64_t o[3];
        for (int k = 0; k < 3; ++k) o[k] = k == a ? c[k] : (c[k] > 0 ? c[k] - 1 : 0);
        float lo = m.at(o[0], o[1], o[2]), hi = lo;
        for (int b = 1; b < 8; ++b) {
            const float w = m.at(o[0] + ((b >> 2) & 1), o[1] + ((b >> 1) & 1), o[2] + (b & 1));
            lo = fminf(lo, w);
            hi = fmaxf(hi, w);
        }
        values[out] = hi - lo;
        ++out;
    }
}

__global__ __launch_bounds__(kMcBlock) void mc_faces_kernel(McVol m, int64_t n, const int64_t* __restrict__ block_v,
                                                            const int64_t* __restrict__ block_f,
                                                            const uint16_t* __restrict__ tag, int descent,
                                                            int* __restrict__ faces) {
    __shared__ int lds[kMcBlock];
    const int64_t i = (int64_t)blockIdx.x * kMcBlock + threadIdx.x;
    int64_t x = 0, y = 0, z = 0;
    int nf = 0;
    mc::Loops L;
    if (i < n) {
        z = i % m.nz; y = (i / m.nz) % m.ny; x = i / (m.nz * m.ny);
        if (is_cube(m, x, y, z)) nf = cube_tris(m, x, y, z, L);
    }
    int total;
    const int local = block_excl_scan(nf, lds, &total);
    if (nf == 0) return;
    int64_t out = block_f[blockIdx.x] + local;
    int pos = 0;
    for (int l = 0; l < L.n_loops; ++l) {
        int id[12];
        for (int k = 0; k < L.len[l]; ++k) {
            const int e = L.edge[pos + k];
            const int cb = mc::edge_corner(e), axis = e >> 2;
            const int64_t j = i + ((cb >> 2) & 1) * m.ny * m.nz + ((cb >> 1) & 1) * m.nz + (cb & 1);
            const int tg = tag[j];
            id[k] = (int)(block_v[j / kMcBlock] + (tg >> 3) + __popc(tg & 7 & ((1 << axis) - 1)));
        }
        for (int k = 1; k + 1 < L.len[l]; ++k) {
            int* f = faces + out * 3;
            f[0] = id[0];
            f[1] = descent ? id[k + 1] : id[k];
            f[2] = descent ? id[k] : id[k + 1];
            ++out;
        }
        pos += L.len[l];
    }
}

// workspace: block_v[nb+1], block_f[nb+1], scan scratch, minmax[2] (int), tag[n] (uint16)
struct McWorkspace {
    int64_t nb, *block_v, *block_f, *scratch;
    int* minmax;
    uint16_t* tag;
};

static int64_t mc_layout(int64_t nx, int64_t ny, int64_t nz, char* base, McWorkspace* w) {
    const int64_t n = nx * ny * nz, nb = div_up(n, kMcBlock);
    int64_t off = 0;
    auto take = [&](int64_t bytes) { const int64_t o = off; off += (bytes + 255) / 256 * 256; return base ? base + o : nullptr; };
    char* bv = take((nb + 1) * 8);
    char* bf = take((nb + 1) * 8);
    char* sc = take(scan_scratch(nb + 1) * 8);
    char* mm = take(2 * sizeof(int));
    char* tg = take(n * 2);
    if (w) {
        w->nb = nb; w->block_v = (int64_t*)bv; w->block_f = (int64_t*)bf; w->scratch = (int64_t*)sc;
        w->minmax = (int*)mm; w->tag = (uint16_t*)tg;
    }
    return off;
}

static bool bad_dims(int64_t nx, int64_t ny, int64_t nz, const char* what) {
    if (nx < 2 || ny < 2 || nz < 2 || nx > (INT64_MAX / 4) / ny / nz) {
        set_error("%s: every axis of the volume needs at least 2 samples", what);
        return true;
    }
    return false;
}

static float unordered(int i) { return __builtin_bit_cast(float, i >= 0 ? i : i ^ 0x7fffffff); }

}  // namespace mi

using namespace mi;

extern "C" {

int64_t mi_mc_workspace_bytes(int64_t nx, int64_t ny, int64_t nz) {
    if (bad_dims(nx, ny, nz, "mi_mc_workspace_bytes")) return MI_EINVAL;
    return mc_layout(nx, ny, nz, nullptr, nullptr);
}

int mi_marching_cubes_count(const float* volume, int64_t nx, int64_t ny, int64_t nz, double level, void* workspace,
                            int64_t* n_verts, int64_t* n_faces, void* stream) {
    if (bad_dims(nx, ny, nz, "mi_marching_cubes_count")) return MI_EINVAL;
    if (!volume || !workspace || !n_verts || !n_faces) { set_error("mi_marching_cubes_count: null pointer argument"); return MI_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    McWorkspace w;
    mc_layout(nx, ny, nz, (char*)workspace, &w);
    const int64_t n = nx * ny * nz;
    const McVol m{volume, nx, ny, nz, level};
    hipLaunchKernelGGL(minmax_init_kernel, dim3(1), dim3(1), 0, s, w.minmax);
    if (hipMemsetAsync(w.block_v + w.nb, 0, 8, s) != hipSuccess || hipMemsetAsync(w.block_f + w.nb, 0, 8, s) != hipSuccess) {
        set_error("mi_marching_cubes_count: %s", hipGetErrorString(hipGetLastError()));
        return MI_EHIP;
    }
    hipLaunchKernelGGL(mc_count_kernel, dim3((unsigned)w.nb), dim3(kMcBlock), 0, s, m, n, w.block_v, w.block_f, w.minmax);
    if (int rc = check_launch("mc_count")) return rc;
    if (int rc = scan_excl(w.block_v, w.nb + 1, w.scratch, s)) return rc;
    if (int rc = scan_excl(w.block_f, w.nb + 1, w.scratch, s)) return rc;
    int64_t tot[2];
    int mm[2];
    if (hipMemcpyAsync(&tot[0], w.block_v + w.nb, 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(&tot[1], w.block_f + w.nb, 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(mm, w.minmax, sizeof(mm), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
        set_error("mi_marching_cubes_count: %s", hipGetErrorString(hipGetLastError()));
        return MI_EHIP;
    }
    const double lo = unordered(mm[0]), hi = unordered(mm[1]);
    if (!(level >= lo && level <= hi)) {
        set_error("Surface level must be within volume data range.");
        return MI_ERANGE;
    }
    if (tot[0] >= ((int64_t)1 << 31)) {
        set_error("mi_marching_cubes_count: %lld vertices do not fit the int32 face indices", (long long)tot[0]);
        return MI_EINVAL;
    }
    *n_verts = tot[0];
    *n_faces = tot[1];
    return MI_OK;
}

int mi_marching_cubes_emit(const float* volume, int64_t nx, int64_t ny, int64_t nz, double level, const double* spacing,
                           int descent, void* workspace, float* verts, int* faces, float* normals, float* values,
                           void* stream) {
    if (bad_dims(nx, ny, nz, "mi_marching_cubes_emit")) return MI_EINVAL;
    if (!volume || !workspace || !spacing || !verts || !faces || !normals || !values) {
        set_error("mi_marching_cubes_emit: null pointer argument");
        return MI_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    McWorkspace w;
    mc_layout(nx, ny, nz, (char*)workspace, &w);
    const int64_t n = nx * ny * nz;
    const McVol m{volume, nx, ny, nz, level};
    hipLaunchKernelGGL(mc_verts_kernel, dim3((unsigned)w.nb), dim3(kMcBlock), 0, s, m, n, w.block_v, spacing[0],
                       spacing[1], spacing[2], verts, normals, values, w.tag);
    if (int rc = check_launch("mc_verts")) return rc;
    hipLaunchKernelGGL(mc_faces_kernel, dim3((unsigned)w.nb), dim3(kMcBlock), 0, s, m, n, w.block_v, w.block_f, w.tag,
                       descent ? 1 : 0, faces);
    return check_launch("mc_faces");
}

}  // extern "C"
