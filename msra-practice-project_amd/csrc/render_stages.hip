// render_stages.hip - the HBM-bound stages around the fused field MLP (gfx950).
//
//   gen_rays_kernel       get_rays                       reference nerf/render.py:7-23
//   sample_coarse_kernel  stratified depths              nerf/render.py:123-132
//   composite_kernel      raw_to_outputs                 nerf/render.py:78-103
//   composite_weights_kernel  its weights (+ depth / acc) from sigma alone, for a coarse pass whose colours are discarded
//   composite_weights_window_kernel  the same, resumable window by window
//   composite_bwd_kernel  autograd of raw_to_outputs
//   sample_fine_kernel    sample_pdf + detach/cat/sort   nerf/render.py:27-56, 140-142
//   sample_pdf_kernel     sample_pdf alone
//   sample_coarse_bounds_kernel / sample_fine_kernel<true>   the two samplers over a range per ray (clipping to an occupancy grid)
//   clear_floats_kernel   zeroes a buffer inside a call's launch sequence, where a captured memset node does not replay
//
// Each computation is stated once: every compositing kernel takes its weights and transmittances from composite_pass
// (with sample_delta and ray_norm) under the G that dispatch_G picks, and both sampling kernels draw through
// normalise_pdf and draw_inverse_cdf.
//
// All arithmetic is fp32 in the reference's operation order (this file is compiled with
// -ffp-contract=off so a*b+c stays two roundings like the un-fused torch/NumPy ops).
// These stages move 20-30 B per sample against 1.2 MFLOP per sample in the MLP: they are
// coalesced streaming kernels, not worth fusing further.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launchers.h"
#include "mi_host.h"
#include "mi_philox.h"

namespace mi {

// ---------------------------------------------------------------------------------------
// get_rays: ray `idx` of the row-major H*W list; dirs = ((i-W/2)/f, -(j-H/2)/f, -1);
// d = sum_k dirs[k]*c2w[c][k] accumulated left to right like np.sum over 3 elements.
// ---------------------------------------------------------------------------------------
struct Cam { float m[12]; };

// T = float reproduces NumPy when `focal` is a Python float (weak scalar -> all-fp32 math);
// T = double reproduces it when `focal` is an np.float64 scalar (pi_GAN/modules.py:127: the
// whole expression is promoted to fp64 and rounded to fp32 by torch.tensor(..., dtype=float)).
template <class T>
__global__ void gen_rays_kernel(int width, T half_w, T half_h, T focal, Cam cam, int64_t ray0, int64_t n,
                                float* __restrict__ rays) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int64_t idx = ray0 + t;
    const T i = (T)(float)(idx % width), j = (T)(float)(idx / width);
    const T d0 = (i - half_w) / focal;
    const T d1 = -((j - half_h) / focal);
    const T d2 = (T)-1;
    float* o = rays + t * 6;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        o[c] = cam.m[4 * c + 3];
        o[3 + c] = (float)((d0 * (T)cam.m[4 * c + 0] + d1 * (T)cam.m[4 * c + 1]) + d2 * (T)cam.m[4 * c + 2]);
    }
}

// ---------------------------------------------------------------------------------------
// linspace(start, end, steps)[i] as ATen's scalar formula (RangeFactories: symmetric halves).
// The host may instead pass the table torch.linspace produced so z matches the CPU oracle
// bit for bit (its vectorised path differs from this formula by 1 ulp on a few entries).
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ float linspace_at(float start, float end, int steps, int i) {
    if (steps <= 1) return start;
    const float step = (end - start) / (float)(steps - 1);
    return i < steps / 2 ? start + step * (float)i : end - step * (float)(steps - i - 1);
}

// The stratified depth of one (ray, sample); the jitter word of sample k of a ray: philox_u32(seed, ray, k) of mi_philox.h.
// kBounds: the linspace runs over the ray's own range bounds[ray] = (near_r, far_r) (mi_occupancy_clip_rays) instead of the
// call's one [near_, far_]; a z_lin table has no meaning per ray and is not read.  Nothing else differs.
template <bool kBounds>
__device__ __forceinline__ void sample_coarse_point(int64_t n, float near_, float far_, const float* __restrict__ bounds, int nc,
                                                    const float* __restrict__ z_lin, const float* __restrict__ t_rand,
                                                    uint64_t seed, uint64_t ray0, float* __restrict__ z) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * nc) return;
    const int k = (int)(t % nc);
    const int64_t ray = t / nc;
    if constexpr (kBounds) { near_ = bounds[ray * 2]; far_ = bounds[ray * 2 + 1]; }
    auto lin = [&](int i) { return !kBounds && z_lin ? z_lin[i] : linspace_at(near_, far_, nc, i); };
    const float zk = lin(k);
    const float lower = k == 0 ? zk : 0.5f * (zk + lin(k - 1));
    const float upper = k == nc - 1 ? zk : 0.5f * (lin(k + 1) + zk);
    const float u = t_rand ? t_rand[t] : (float)(philox_u32(seed, ray0 + (uint64_t)ray, (uint32_t)k) >> 8) * 0x1p-24f;
    z[t] = lower + (upper - lower) * u;
}

__global__ void sample_coarse_kernel(int64_t n, float near_, float far_, int nc, const float* __restrict__ z_lin,
                                     const float* __restrict__ t_rand, uint64_t seed, uint64_t ray0,
                                     float* __restrict__ z) {
    sample_coarse_point<false>(n, near_, far_, nullptr, nc, z_lin, t_rand, seed, ray0, z);
}

__global__ void sample_coarse_bounds_kernel(int64_t n, const float* __restrict__ bounds, int nc, const float* __restrict__ t_rand,
                                            uint64_t seed, uint64_t ray0, float* __restrict__ z) {
    sample_coarse_point<true>(n, 0.f, 0.f, bounds, nc, nullptr, t_rand, seed, ray0, z);
}

// ---------------------------------------------------------------------------------------
// composite (raw_to_outputs): G lanes per ray (G = 16/32/64), lane = sample, passes of G samples with the transmittance
// carried between passes.  alpha = 1-exp(-sigma*delta*|d|), T = exclusive prod(1-alpha+1e-10), w = alpha*T;
// rgb = sum w c + (1-acc) (white background).  Every kernel that needs weights or transmittances - the two one-pass
// forwards, the windowed forward, sweep 1 of the backward - gets them from composite_pass below and from nowhere else,
// so they all hold the same bits for the same samples under the same G.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ float ray_norm(const float* rays, int64_t ray) {
    const float* rd = rays + ray * 6 + 3;
    return sqrtf((rd[0] * rd[0] + rd[1] * rd[1]) + rd[2] * rd[2]);
}

// delta * |d| of sample kc of a ray's S depths, zp = the address of its own depth: the distance to the next sample,
// "infinity" behind the last one
__device__ __forceinline__ float sample_delta(const float* zp, int S, int kc, float nrm) {
    const float zk = zp[0];
    const float zn = kc + 1 < S ? zp[1] : 0.f;
    const float delta = kc + 1 < S ? zn - zk : 1e10f;
    return delta * nrm;
}

struct PassOut {
    float w;        // alpha * trans
    float trans;    // the transmittance in front of the sample, (float)(T * exclusive product)
    double p;       // inclusive product of the pass's factors up to this lane; lane G-1 holds the whole pass's
};

// One pass of G samples, lane `sub` holding one (in = false: a lane past the row's end, the factor 1 and w = 0), T the
// product of all earlier passes.  The running product is kept in fp64 and rounded to fp32 per sample, as ATen's CPU
// cumprod does (accumulate type of float is double).  The caller carries T = T * __shfl(p, G - 1, G).
template <int G>
__device__ __forceinline__ PassOut composite_pass(int sub, bool in, float sigma, float delta, double T) {
    const float alpha = in ? 1.0f - expf(-sigma * delta) : 0.f;
    const float f = in ? (1.0f - alpha) + 1e-10f : 1.f;
    double p = (double)f;
#pragma unroll
    for (int o = 1; o < G; o <<= 1) {
        const double q = __shfl_up(p, o, G);
        if (sub >= o) p *= q;
    }
    double excl = __shfl_up(p, 1, G);
    if (sub == 0) excl = 1.0;
    const float trans = (float)(T * excl);
    return {alpha * trans, trans, p};
}

// The one-pass forward.  kColour: src = raw [n,S,4], all five sums, rgb / depth / acc written, weights when non-null.
// Otherwise the coarse pass of a renderer that discards the coarse colours: only sigma is read (element e at
// src[e * sigma_stride]: a compact [n,S] buffer with stride 1, or the sigma channel of raw with raw + 3 and stride 4),
// the weights [n,S] are written, depth / acc only when non-null (the colour sums it drops are sums of their own).
template <int G, bool kColour>
__device__ __forceinline__ void composite_rows(int64_t n, int S, const float* src, int sigma_stride,
                                               const float* z, const float* rays,
                                               float* rgb, float* depth,
                                               float* acc, float* weights) {
    const int lane = threadIdx.x & 63;
    const int sub = lane & (G - 1);
    const int64_t groups_per_block = 256 / G;
    const int64_t ray = (int64_t)blockIdx.x * groups_per_block + threadIdx.x / G;
    const bool live = ray < n;
    const int64_t rc = live ? ray : n - 1;
    const float nrm = ray_norm(rays, rc);
    double T = 1.0;
    float sr = 0.f, sg = 0.f, sb = 0.f, sd = 0.f, sa = 0.f;
    for (int k0 = 0; k0 < S; k0 += G) {
        const int k = k0 + sub;
        const bool in = k < S;
        const int kc = in ? k : S - 1;
        float4 c;
        if constexpr (kColour) c = reinterpret_cast<const float4*>(src)[rc * S + kc];
        else c.w = src[(rc * S + kc) * sigma_stride];
        const float* zp = z + (rc * S + kc);
        const float zk = *zp;
        const PassOut o = composite_pass<G>(sub, in, c.w, sample_delta(zp, S, kc, nrm), T);
        T = T * __shfl(o.p, G - 1, G);
        if (in) {
            if constexpr (kColour) { sr += o.w * c.x; sg += o.w * c.y; sb += o.w * c.z; }
            sd += o.w * zk; sa += o.w;
            if ((!kColour || weights) && live) weights[rc * S + k] = o.w;
        }
    }
    if (!kColour && !depth && !acc) return;
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) {
        if constexpr (kColour) { sr += __shfl_xor(sr, o, G); sg += __shfl_xor(sg, o, G); sb += __shfl_xor(sb, o, G); }
        sd += __shfl_xor(sd, o, G); sa += __shfl_xor(sa, o, G);
    }
    if (live && sub == 0) {
        if constexpr (kColour) {
            const float bg = 1.0f - sa;
            rgb[ray * 3 + 0] = sr + bg; rgb[ray * 3 + 1] = sg + bg; rgb[ray * 3 + 2] = sb + bg;
        }
        if (kColour || depth) depth[ray] = sd;
        if (kColour || acc) acc[ray] = sa;
    }
}

// the two forms under the names kernel traces know them by
template <int G>
__global__ __launch_bounds__(256) void composite_kernel(int64_t n, int S, const float* __restrict__ raw,
                                                        const float* __restrict__ z, const float* __restrict__ rays,
                                                        float* __restrict__ rgb, float* __restrict__ depth,
                                                        float* __restrict__ acc, float* __restrict__ weights) {
    composite_rows<G, true>(n, S, raw, 4, z, rays, rgb, depth, acc, weights);
}

template <int G>
__global__ __launch_bounds__(256) void composite_weights_kernel(int64_t n, int S, const float* __restrict__ sigma,
                                                                int sigma_stride, const float* __restrict__ z,
                                                                const float* __restrict__ rays, float* __restrict__ depth,
                                                                float* __restrict__ acc, float* __restrict__ weights) {
    composite_rows<G, false>(n, S, sigma, sigma_stride, z, rays, nullptr, depth, acc, weights);
}

// The weights form made resumable, for a coarse pass evaluated front to back in windows of samples (mi_render_rays): the
// call behind the window [k0, k1) runs the passes over samples [0, k1) of every live ray under dispatch_G's G for S, a
// sample >= k1 standing in as w = 0, and writes the weights of [k0, k1).  Then it decides the ray against `stop`, the
// caller's threshold (launchers.h: kStopZeroWeight = 2^-151, or kStopBelowPdfEps = 2^-42 when sample_fine is the weights'
// only reader - the argument why it then sees the same bits stands there).  With 2^-151:
//   * D, the fp64 running product in front of sample k1, is <= 2^-151: every later sample's (float)(T * excl) is 0.0f
//     whatever its sigma is.  The factors f = (1-alpha)+1e-10f are <= 1 (sigma >= 0, ascending depths), so the exact
//     product can only fall; the scans' products of <= 2G factors differ from the exact ones by a relative 2^-45 at most,
//     far inside the factor 2 between 2^-151 and the largest double that still rounds to 0.0f, 2^-150.  Such a ray is
//     FINISHED: zero weights behind k1, depth / acc from the sums so far - the one-pass kernel adds w * z = 0 and
//     w = 0 for those samples, which changes no bit of either sum.  Nothing behind k1 is read: no field evaluation there.
//   * otherwise the ray goes to live_out for the next window (one atomic per block; the list's order is arbitrary and
//     touches no output: a ray's results depend on its own samples alone).
// live_out null = the last window (k1 = S): every ray is finished.  Blocks past the live count return at once.
// Recomputing [0, k0) from the stored sigma instead of carrying T and the partial sums costs a few reads of a buffer
// that the pass just wrote and keeps the partition of samples into passes the one-pass kernel's.
constexpr int kWindowIter = 8;                        // entries per G-lane group: (256 / G) * kWindowIter entries per block

template <int G>
__global__ __launch_bounds__(256) void composite_weights_window_kernel(
    int64_t n, int S, const float* __restrict__ sigma, const float* __restrict__ z, const float* __restrict__ rays,
    float* __restrict__ depth, float* __restrict__ acc, float* __restrict__ weights, const int* __restrict__ live_in,
    const int* __restrict__ count_in, int* __restrict__ live_out, int* __restrict__ count_out, int k0, int k1,
    double stop) {
    constexpr int kPerBlock = 256 / G * kWindowIter;
    __shared__ int s_keep[kPerBlock];
    __shared__ int s_n, s_base;
    const int64_t count = count_in ? (int64_t)*count_in : n;
    const int64_t first = (int64_t)blockIdx.x * kPerBlock;
    if (first >= count) return;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int sub = lane & (G - 1);
    for (int it = 0; it < kWindowIter; ++it) {
        const int64_t entry = first + (int64_t)it * (256 / G) + threadIdx.x / G;
        const bool live = entry < count;
        const int64_t rc = live ? (live_in ? (int64_t)live_in[entry] : entry) : 0;
        const float nrm = ray_norm(rays, rc);
        double T = 1.0, D = 1.0;
        float sd = 0.f, sa = 0.f;
        for (int kk = 0; kk < k1; kk += G) {
            const int k = kk + sub;
            const bool in = k < k1;
            const int kc = in ? k : k1 - 1;
            const float sg = sigma[rc * S + kc];
            const float zk = z[rc * S + kc];
            const PassOut o = composite_pass<G>(sub, in, sg, sample_delta(z + (rc * S + kc), S, kc, nrm), T);
            if (kk + G >= k1) D = T * __shfl(o.p, k1 - 1 - kk, G);     // the product in front of sample k1
            T = T * __shfl(o.p, G - 1, G);
            if (in) {
                sd += o.w * zk; sa += o.w;
                if (live && k >= k0) weights[rc * S + k] = o.w;
            }
        }
        const bool done = !live_out || D <= stop;
        if (live && !done && sub == 0) s_keep[atomicAdd(&s_n, 1)] = (int)rc;
        if (live && done)
            for (int k = k1 + sub; k < S; k += G) weights[rc * S + k] = 0.f;
        if (done && (depth || acc)) {
#pragma unroll
            for (int o = G / 2; o > 0; o >>= 1) {
                sd += __shfl_xor(sd, o, G); sa += __shfl_xor(sa, o, G);
            }
            if (live && sub == 0) {
                if (depth) depth[rc] = sd;
                if (acc) acc[rc] = sa;
            }
        }
    }
    if (!live_out) return;
    __syncthreads();
    if (threadIdx.x == 0) s_base = s_n ? atomicAdd(count_out, s_n) : 0;
    __syncthreads();
    for (int i = threadIdx.x; i < s_n; i += 256) live_out[s_base + i] = s_keep[i];
}

// ---------------------------------------------------------------------------------------
// composite backward (autograd of raw_to_outputs, render.py:91-101): G lanes per ray, lane = sample.
//   Gk = sum_c g_rgb[c]*(c_k[c]-1) + g_depth*z_k + g_acc        (dL/dw_k; rgb carries +1-acc)
//   dL/dalpha_k = T_k * (Gk - S_k),  S_k = sum_{j>k} Gj alpha_j prod_{k<i<j} f_i = R_{k+1} with the
//                 division-free first-order recurrence R_k = Gk alpha_k + f_k R_{k+1}
//   dL/dsigma_k = dL/dalpha_k * delta_k * (1-alpha_k);   dL/dc_k = g_rgb * w_k
// f_k = 1-alpha_k+1e-10.  z and rays carry no gradient (z_samples is detached, render.py:141).
// Sweep 1 (passes of G samples, front to back): the forward's transmittance T_k (composite_pass), parked in the
// output's .w slot.  Sweep 2 (back to front): R by a reverse scan of the affine maps (f_k, Gk alpha_k) inside the
// pass, carried between passes.
// ---------------------------------------------------------------------------------------
template <int G>
__global__ __launch_bounds__(256) void composite_bwd_kernel(int64_t n, int S, const float* __restrict__ raw,
                                                            const float* __restrict__ z,
                                                            const float* __restrict__ rays,
                                                            const float* __restrict__ g_rgb,
                                                            const float* __restrict__ g_depth,
                                                            const float* __restrict__ g_acc,
                                                            const float* __restrict__ g_w,
                                                            float* __restrict__ g_raw) {
    const int lane = threadIdx.x & 63;
    const int sub = lane & (G - 1);
    const int64_t ray = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    const bool live = ray < n;
    const int64_t rc = live ? ray : n - 1;
    const float nrm = ray_norm(rays, rc);
    const float gr = g_rgb ? g_rgb[rc * 3 + 0] : 0.f, gg = g_rgb ? g_rgb[rc * 3 + 1] : 0.f,
                gb = g_rgb ? g_rgb[rc * 3 + 2] : 0.f;
    const float gd = g_depth ? g_depth[rc] : 0.f, ga = g_acc ? g_acc[rc] : 0.f;
    const float4* rw = reinterpret_cast<const float4*>(raw) + rc * S;
    const float* zr = z + rc * S;
    float4* out = reinterpret_cast<float4*>(g_raw) + rc * S;
    const int passes = (S + G - 1) / G;
    double T = 1.0;
    for (int pass = 0; pass < passes; ++pass) {
        const int k = pass * G + sub;
        const bool in = k < S;
        const int kc = in ? k : S - 1;
        const PassOut o = composite_pass<G>(sub, in, rw[kc].w, sample_delta(zr + kc, S, kc, nrm), T);
        if (in && live) out[k].w = o.trans;
        T = T * __shfl(o.p, G - 1, G);
    }
    float carry = 0.f;                                   // R at the first sample of the pass behind this one
    for (int pass = passes - 1; pass >= 0; --pass) {
        const int k = pass * G + sub;
        const bool in = k < S;
        const int kc = in ? k : S - 1;
        const float4 c = rw[kc];
        const float zk = zr[kc];
        const float delta = sample_delta(zr + kc, S, kc, nrm);
        const float e = expf(-c.w * delta);
        const float alpha = 1.0f - e;
        const float Tk = in && live ? out[kc].w : 0.f;
        // dL/dw_k; g_w = the cotangent of the returned weights themselves (raw_to_outputs hands them out, render.py:103)
        float Gk = gr * (c.x - 1.f) + gg * (c.y - 1.f) + gb * (c.z - 1.f) + gd * zk + ga;
        if (g_w) Gk += g_w[rc * S + kc];
        // affine map of this sample, R_k = A + M * R_{k+1}; composed towards higher lanes
        float M = in ? (1.0f - alpha) + 1e-10f : 1.f, A = in ? Gk * alpha : 0.f;
#pragma unroll
        for (int o = 1; o < G; o <<= 1) {
            const float M2 = __shfl_down(M, o, G), A2 = __shfl_down(A, o, G);
            if (sub + o < G) { A = A + M * A2; M = M * M2; }
        }
        const float R = A + M * carry;                   // R_k
        float Snext = __shfl_down(R, 1, G);              // S_k = R_{k+1}
        if (sub == G - 1) Snext = carry;
        carry = __shfl(R, 0, G);
        if (in && live) {
            const float w = alpha * Tk;
            const float dalpha = Tk * (Gk - Snext);
            out[k] = make_float4(gr * w, gg * w, gb * w, dalpha * delta * e);
        }
    }
}

// ---------------------------------------------------------------------------------------
// composite backward towards the ray direction: the part of raw_to_outputs' autograd that composite_bwd_kernel leaves
// out.  render.py:91-93: dists = delta_z * |d|, alpha = 1 - exp(-sigma * dists), so
//   dL/d|d| = sum_k ((dL/dalpha_k * exp(-sigma_k dists_k)) * sigma_k) * delta_z_k      (autograd's order of products)
//   dL/dd   = dL/d|d| * d / |d|                                                         (torch.norm's backward)
// with dL/dalpha_k exactly as in composite_bwd_kernel (same two sweeps, the transmittances parked in LDS instead of
// the output).  The last interval's delta_z is 1e10 like the reference's: sigma = 0 gives (x * 0) * 1e10 = 0, sigma > 0
// gives exp(-huge) = 0, both finite.  z carries no gradient (render.py:141), the origin none from compositing.
// accumulate = 0 writes the ray's six floats (g_o = 0), otherwise the three of g_d are added to.
// ---------------------------------------------------------------------------------------
template <int G>
__global__ __launch_bounds__(256) void composite_bwd_rays_kernel(int64_t n, int S, const float* __restrict__ raw,
                                                                 const float* __restrict__ z,
                                                                 const float* __restrict__ rays,
                                                                 const float* __restrict__ g_rgb,
                                                                 const float* __restrict__ g_depth,
                                                                 const float* __restrict__ g_acc,
                                                                 const float* __restrict__ g_w, int accumulate,
                                                                 float* __restrict__ g_rays) {
    extern __shared__ float s_trans[];                   // [256 / G][S]
    const int lane = threadIdx.x & 63;
    const int sub = lane & (G - 1);
    const int64_t ray = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    const bool live = ray < n;
    const int64_t rc = live ? ray : n - 1;
    const float nrm = ray_norm(rays, rc);
    const float gr = g_rgb ? g_rgb[rc * 3 + 0] : 0.f, gg = g_rgb ? g_rgb[rc * 3 + 1] : 0.f,
                gb = g_rgb ? g_rgb[rc * 3 + 2] : 0.f;
    const float gd = g_depth ? g_depth[rc] : 0.f, ga = g_acc ? g_acc[rc] : 0.f;
    const float4* rw = reinterpret_cast<const float4*>(raw) + rc * S;
    const float* zr = z + rc * S;
    float* tr = s_trans + (int64_t)(threadIdx.x / G) * S;
    const int passes = (S + G - 1) / G;
    double T = 1.0;
    for (int pass = 0; pass < passes; ++pass) {
        const int k = pass * G + sub;
        const bool in = k < S;
        const int kc = in ? k : S - 1;
        const PassOut o = composite_pass<G>(sub, in, rw[kc].w, sample_delta(zr + kc, S, kc, nrm), T);
        if (in) tr[k] = o.trans;
        T = T * __shfl(o.p, G - 1, G);
    }
    float carry = 0.f, gn = 0.f;
    for (int pass = passes - 1; pass >= 0; --pass) {
        const int k = pass * G + sub;
        const bool in = k < S;
        const int kc = in ? k : S - 1;
        const float4 c = rw[kc];
        const float zk = zr[kc];
        const float dz = kc + 1 < S ? zr[kc + 1] - zk : 1e10f;
        const float e = expf(-c.w * sample_delta(zr + kc, S, kc, nrm));
        const float alpha = 1.0f - e;
        const float Tk = in ? tr[kc] : 0.f;
        float Gk = gr * (c.x - 1.f) + gg * (c.y - 1.f) + gb * (c.z - 1.f) + gd * zk + ga;
        if (g_w) Gk += g_w[rc * S + kc];
        float M = in ? (1.0f - alpha) + 1e-10f : 1.f, A = in ? Gk * alpha : 0.f;
#pragma unroll
        for (int o = 1; o < G; o <<= 1) {
            const float M2 = __shfl_down(M, o, G), A2 = __shfl_down(A, o, G);
            if (sub + o < G) { A = A + M * A2; M = M * M2; }
        }
        const float R = A + M * carry;
        float Snext = __shfl_down(R, 1, G);
        if (sub == G - 1) Snext = carry;
        carry = __shfl(R, 0, G);
        if (in) gn += ((Tk * (Gk - Snext) * e) * c.w) * dz;
    }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) gn += __shfl_xor(gn, o, G);
    if (live && sub < 6) {
        const float* rd = rays + ray * 6 + 3;
        float* out = g_rays + ray * 6 + sub;
        const float v = sub < 3 ? 0.f : gn * rd[sub - 3] / nrm;
        if (!accumulate) *out = v;
        else if (sub >= 3) *out += v;
    }
}

// ---------------------------------------------------------------------------------------
// cdf[j] = fp32(sum_{i<j} pdf[i]) with the running sum in fp64, j = 0..nb-1, pdf[0..nb-2] in LDS: ATen's CPU cumsum
// keeps the running sum in the accumulate type of float, i.e. DOUBLE, and rounds every output to fp32
// (cpu_cum_base_kernel).  A double holds every partial sum of these floats EXACTLY whenever the terms' exponents span
// few enough bits (largest sum's exponent - smallest term's last mantissa bit <= 52), and exact sums do not depend
// on the order of the additions: the wave then takes a shuffle scan (6 steps) instead of nb dependent additions.
// Terms that do not qualify (inf / NaN, or a dynamic range beyond 2^(28 - log2 nb)) take the sequential order itself.
// The bits a sum needs: fmax - fmin for the span of the exponent fields (a denormal counts as field 1, where its last bit
// lies), 24 for a term's mantissa, log2n = bit_length(nb - 1) for adding nb - 1 < 2^log2n terms: 52 at the criterion's edge.
// The criterion is one bit stricter than a double's 53 demand: no row with fmax - fmin = 29 - log2n can tell the two orders
// apart either; at 30 - log2n one can (nb = 64; tests/test_sampler_ref_host.py holds both rows and the integer proof).
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void cdf_like_cumsum(const float* pdf, float* cdf, int nb, int lane) {
    const int nw = nb - 1;
    int fmin = 255, fmax = 0;
    for (int j = lane; j < nw; j += 64) {
        const int f = (int)((__float_as_uint(pdf[j]) >> 23) & 0xffu);
        const bool zero = (__float_as_uint(pdf[j]) << 1) == 0u;
        fmax = f > fmax ? f : fmax;
        if (!zero) { const int g = f > 1 ? f : 1; fmin = g < fmin ? g : fmin; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int a = __shfl_xor(fmin, o), b = __shfl_xor(fmax, o);
        fmin = a < fmin ? a : fmin;
        fmax = b > fmax ? b : fmax;
    }
    const int log2n = 32 - __builtin_clz((unsigned)(nb > 1 ? nb - 1 : 1));
    const bool exact = fmax < 255 && (fmin > fmax || fmax - fmin <= 28 - log2n);
    if (exact) {
        double carry = 0.0;
        for (int base = 0; base < nb; base += 64) {
            const int j = base + lane;
            double incl = j < nw ? (double)pdf[j] : 0.0;
            const double own = incl;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const double up = __shfl_up(incl, o);
                if (lane >= o) incl += up;
            }
            if (j < nb) cdf[j] = (float)(carry + (incl - own));      // exclusive prefix (exact, like every sum here)
            carry += __shfl(incl, 63);
        }
    } else {
        for (int j = lane; j < nb; j += 64) {
            double sum = 0.0;
            for (int i = 0; i < j; ++i) sum += (double)pdf[i];
            cdf[j] = (float)sum;
        }
    }
}

// (value, index) as one unsigned key: float order for everything that is not a NaN (with -0 before +0), ties by
// index - the rank sort below then needs one 64-bit compare per pair instead of two float compares and an index test
__device__ __forceinline__ uint64_t sort_key(float v, int i) {
    uint32_t b = __float_as_uint(v);
    b ^= (b >> 31) ? 0xffffffffu : 0x80000000u;
    return ((uint64_t)b << 32) | (uint32_t)i;
}

// ---------------------------------------------------------------------------------------
// The inverse-CDF draw of sample_pdf (render.py:27-56), one wave per ray, in two parts around cdf_like_cumsum.
// pdf[j] = (w[j] + kPdfEps) / sum_j (w[j] + kPdfEps), j < nw, kPdfEps = 1e-5 (launchers.h): strided partial sums, xor
// reduction, one division per entry.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void normalise_pdf(const float* __restrict__ w, int nw, int lane, float* pdf) {
    float part = 0.f;
    for (int j = lane; j < nw; j += 64) part += w[j] + kPdfEps;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
    for (int j = lane; j < nw; j += 64) pdf[j] = (w[j] + kPdfEps) / part;
}

// the sample at u: idx = #(cdf <= u) (searchsorted right=True on the ascending cdf [nb]), both neighbours clamped into
// the table, a cdf step below 1e-5 replaced by 1, then the lerp between the two bins
__device__ __forceinline__ float draw_inverse_cdf(const float* cdf, const float* bins, int nb, float u) {
    int lo_i = 0, hi_i = nb;
    while (lo_i < hi_i) {
        const int mid = (lo_i + hi_i) >> 1;
        if (cdf[mid] <= u) lo_i = mid + 1; else hi_i = mid;
    }
    const int below = lo_i - 1 > 0 ? lo_i - 1 : 0;
    const int above = lo_i < nb - 1 ? lo_i : nb - 1;
    const float c0 = cdf[below], c1 = cdf[above];
    float denom = c1 - c0;
    if (denom < 1e-5f) denom = 1.f;
    const float t = (u - c0) / denom;
    const float b0 = bins[below], b1 = bins[above];
    return b0 + t * (b1 - b0);
}

// ---------------------------------------------------------------------------------------
// sample_fine: one wave per ray.  bins = mids of the coarse linspace, w = weights[1:-1]+1e-5,
// pdf = w/sum(w) (normalise_pdf), cdf = [0, cumsum(pdf)] with the running sum in fp64 rounded per entry like
// torch.cumsum on CPU; u = linspace(0,1,Nf), each drawn by draw_inverse_cdf;
// then z_fine = sort(cat(z_coarse, z_samples)) by full rank counting (no sortedness assumed; -0 ranks before +0).
// LDS per wave: cdf[Nc] | bins[Nc] | zall[Nc+Nf] | zout[Nc+Nf] (the sorted row, stored coalesced)
// kBounds (sample_fine_bounds_kernel below): the coarse linspace runs over the ray's own range (near_r, far_r)
// (mi_occupancy_clip_rays), so the bins are formed per ray, not once per wave in front of the ray loop.  A z_lin table has no
// meaning per ray, and its parameter carries the bounds [n,2] instead; near_ / far_ arrive unused.  The bins of a ray are
// written behind the closing barrier of the ray before it and first read behind two more.  The flag is on the kernel itself,
// not on a device function under two kernels: inlined into a wrapper, the plain instance came out scheduled differently.
// ---------------------------------------------------------------------------------------
template <bool kBounds>
__global__ __launch_bounds__(256) void sample_fine_kernel(int64_t n, float near_, float far_, int nc, int nf,
                                                          const float* __restrict__ z_lin,
                                                          const float* __restrict__ u_lin,
                                                          const float* __restrict__ z_coarse,
                                                          const float* __restrict__ weights,
                                                          float* __restrict__ z_samples, float* __restrict__ z_fine,
                                                          int* __restrict__ pos) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int S = nc + nf;
    const int per_wave = 2 * nc + 2 * S;
    float* cdf = smem + wave * per_wave;
    float* bins = cdf + nc;
    float* zall = bins + nc;
    float* zout = zall + S;
    const int nb = nc - 1;      // bins / cdf entries
    const int nw = nc - 2;      // interior weights
    auto lin = [&](int i) { return !kBounds && z_lin ? z_lin[i] : linspace_at(near_, far_, nc, i); };
    if constexpr (!kBounds)
        for (int j = lane; j < nb; j += 64) bins[j] = 0.5f * (lin(j + 1) + lin(j));

    for (int64_t ray = (int64_t)blockIdx.x * 4 + wave; ray < n; ray += (int64_t)gridDim.x * 4) {
        const float* wr = weights + ray * nc;
        const float* zc = z_coarse + ray * nc;
        if constexpr (kBounds) {
            near_ = z_lin[ray * 2]; far_ = z_lin[ray * 2 + 1];             // the bounds table
            for (int j = lane; j < nb; j += 64) bins[j] = 0.5f * (lin(j + 1) + lin(j));
        }
        // pdf of the interior weights into zall (scratch), then per-entry sequential prefix = torch.cumsum order
        normalise_pdf(wr + 1, nw, lane, zall);
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        cdf_like_cumsum(zall, cdf, nb, lane);
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        // coarse depths first, then inverse-CDF samples
        for (int j = lane; j < nc; j += 64) zall[j] = zc[j];
        for (int s = lane; s < nf; s += 64) {
            const float zs = draw_inverse_cdf(cdf, bins, nb, u_lin ? u_lin[s] : linspace_at(0.f, 1.f, nf, s));
            zall[nc + s] = zs;
            if (z_samples) z_samples[ray * nf + s] = zs;
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        // Merge by rank: position of an element = #(keys below its own), key = (value, index).  Both lists are
        // sorted on every call the render path makes (stratified depths; inverse-CDF samples of an ascending u), and
        // then a rank is the element's own index in its list plus one binary search in the other list.  A ray whose
        // lists are not sorted (the stage-level entry point takes any depths) is ranked by full counting instead.
        // The two agree wherever both apply, but for a sample of -0 next to a coarse depth of +0 (float compares hold them
        // equal and put the coarse depth first, the key puts -0 first); ascending bins never draw a -0.
        bool sorted = true;
        for (int e = lane; e + 1 < S; e += 64)
            if (e + 1 != nc) sorted = sorted && !(zall[e + 1] < zall[e]) && zall[e] == zall[e] && zall[e + 1] == zall[e + 1];
        if (__builtin_amdgcn_ballot_w64(!sorted) == 0ull) {
            for (int e = lane; e < S; e += 64) {
                const float v = zall[e];
                const bool coarse = e < nc;
                // coarse element: #(samples < v) (an equal sample has the higher index); sample: #(coarse <= v)
                const float* other = coarse ? zall + nc : zall;
                int lo_i = 0, hi_i = coarse ? nf : nc;
                while (lo_i < hi_i) {
                    const int mid = (lo_i + hi_i) >> 1;
                    const float o = other[mid];
                    if (coarse ? o < v : o <= v) lo_i = mid + 1; else hi_i = mid;
                }
                zout[(coarse ? e : e - nc) + lo_i] = v;
                if (pos) pos[ray * S + e] = (coarse ? e : e - nc) + lo_i;
            }
        } else {
            for (int e0 = lane; e0 < S; e0 += 256) {                 // up to four elements per sweep over the list
                uint64_t key[4];
                int rank[4] = {0, 0, 0, 0};
#pragma unroll
                for (int k = 0; k < 4; ++k) key[k] = e0 + 64 * k < S ? sort_key(zall[e0 + 64 * k], e0 + 64 * k) : ~0ull;
#pragma unroll 8
                for (int i = 0; i < S; ++i) {
                    const uint64_t o = sort_key(zall[i], i);
#pragma unroll
                    for (int k = 0; k < 4; ++k) rank[k] += o < key[k] ? 1 : 0;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (e0 + 64 * k < S) {
                        zout[rank[k]] = zall[e0 + 64 * k];
                        if (pos) pos[ray * S + e0 + 64 * k] = rank[k];
                    }
            }
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        for (int e = lane; e < S; e += 64) z_fine[ray * S + e] = zout[e];        // coalesced rows out of LDS
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
}


// ---------------------------------------------------------------------------------------
// sample_pdf as a free-standing function (render.py:27-56) on arbitrary per-ray bins: one wave per ray,
// sample_fine_kernel's draw without the merge.  bins [n,nb], weights [n,nb-1] -> out [n,ns].
// LDS per wave: cdf[nb] | pdf[nb]
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sample_pdf_kernel(int64_t n, int nb, int ns, const float* __restrict__ bins,
                                                         const float* __restrict__ weights,
                                                         const float* __restrict__ u_lin, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* cdf = smem + wave * 2 * nb;
    float* pdf = cdf + nb;
    const int nw = nb - 1;
    for (int64_t ray = (int64_t)blockIdx.x * 4 + wave; ray < n; ray += (int64_t)gridDim.x * 4) {
        const float* wr = weights + ray * nw;
        const float* br = bins + ray * nb;
        normalise_pdf(wr, nw, lane, pdf);
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        cdf_like_cumsum(pdf, cdf, nb, lane);
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        for (int s = lane; s < ns; s += 64)
            out[ray * ns + s] = draw_inverse_cdf(cdf, br, nb, u_lin ? u_lin[s] : linspace_at(0.f, 1.f, ns, s));
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
}

// ---- host launchers ------------------------------------------------------------------------
int launch_gen_rays(int width, int height, double focal, const float* c2w, int64_t ray0, int64_t n, float* rays,
                    int compute_f64, hipStream_t stream) {
    if (n <= 0) return 0;
    Cam cam;
    for (int i = 0; i < 12; ++i) cam.m[i] = c2w[i];
    const unsigned blocks = (unsigned)((n + 255) / 256);
    if (compute_f64)
        hipLaunchKernelGGL(gen_rays_kernel<double>, dim3(blocks), dim3(256), 0, stream, width, width * 0.5,
                           height * 0.5, focal, cam, ray0, n, rays);
    else
        hipLaunchKernelGGL(gen_rays_kernel<float>, dim3(blocks), dim3(256), 0, stream, width, (float)(width * 0.5),
                           (float)(height * 0.5), (float)focal, cam, ray0, n, rays);
    return check_launch("gen_rays");
}

int launch_sample_coarse(int64_t n, float near_, float far_, int nc, const float* z_lin, const float* t_rand,
                         uint64_t seed, uint64_t ray0, float* z, hipStream_t stream) {
    if (n <= 0) return 0;
    const int64_t total = n * nc;
    hipLaunchKernelGGL(sample_coarse_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, n, near_,
                       far_, nc, z_lin, t_rand, seed, ray0, z);
    return check_launch("sample_coarse");
}

int launch_sample_coarse_bounds(int64_t n, const float* bounds, int nc, const float* t_rand, uint64_t seed, uint64_t ray0,
                                float* z, hipStream_t stream) {
    if (n <= 0) return 0;
    const int64_t total = n * nc;
    hipLaunchKernelGGL(sample_coarse_bounds_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, n, bounds, nc,
                       t_rand, seed, ray0, z);
    return check_launch("sample_coarse_bounds");
}

// The lanes per ray of every compositing kernel for rows of S samples, as a compile-time constant: f(integral_constant<G>).
// One choice for all of them: the windowed forward and the backward must cut the samples into the one-pass forward's passes.
template <class F>
static void dispatch_G(int S, F&& f) {
    if (S > 32) f(std::integral_constant<int, 64>{});
    else if (S > 16) f(std::integral_constant<int, 32>{});
    else f(std::integral_constant<int, 16>{});
}

// blocks of 256 threads for n rays (or worst-case list entries), `iter` of them per G-lane group
template <int G>
static dim3 ray_grid(int64_t n, int iter = 1) {
    const int64_t per_block = 256 / G * iter;
    return dim3((unsigned)((n + per_block - 1) / per_block));
}

int launch_composite(int64_t n, int S, const float* raw, const float* z, const float* rays, float* rgb, float* depth,
                     float* acc, float* weights, hipStream_t stream) {
    if (n <= 0) return 0;
    dispatch_G(S, [&](auto g) {
        constexpr int G = decltype(g)::value;
        hipLaunchKernelGGL(composite_kernel<G>, ray_grid<G>(n), dim3(256), 0, stream, n, S, raw, z, rays, rgb, depth, acc,
                           weights);
    });
    return check_launch("composite");
}

int launch_composite_weights(int64_t n, int S, const float* sigma, int sigma_stride, const float* z, const float* rays,
                             float* depth, float* acc, float* weights, hipStream_t stream) {
    if (n <= 0) return 0;
    dispatch_G(S, [&](auto g) {
        constexpr int G = decltype(g)::value;
        hipLaunchKernelGGL(composite_weights_kernel<G>, ray_grid<G>(n), dim3(256), 0, stream, n, S, sigma, sigma_stride, z,
                           rays, depth, acc, weights);
    });
    return check_launch("composite_weights");
}

int launch_composite_weights_window(int64_t n, int S, const float* sigma, const float* z, const float* rays, float* depth,
                                    float* acc, float* weights, const int* live_in, const int* count_in, int* live_out,
                                    int* count_out, int k0, int k1, double stop, hipStream_t stream) {
    if (n <= 0) return 0;
    dispatch_G(S, [&](auto g) {                          // grid: the worst case, every ray live
        constexpr int G = decltype(g)::value;
        hipLaunchKernelGGL(composite_weights_window_kernel<G>, ray_grid<G>(n, kWindowIter), dim3(256), 0, stream, n, S,
                           sigma, z, rays, depth, acc, weights, live_in, count_in, live_out, count_out, k0, k1,
                           stop);
    });
    return check_launch("composite_weights_window");
}

int launch_composite_bwd(int64_t n, int S, const float* raw, const float* z, const float* rays, const float* g_rgb,
                         const float* g_depth, const float* g_acc, const float* g_w, float* g_raw, hipStream_t stream) {
    if (n <= 0) return 0;
    dispatch_G(S, [&](auto g) {
        constexpr int G = decltype(g)::value;
        hipLaunchKernelGGL(composite_bwd_kernel<G>, ray_grid<G>(n), dim3(256), 0, stream, n, S, raw, z, rays, g_rgb, g_depth,
                           g_acc, g_w, g_raw);
    });
    return check_launch("composite_bwd");
}

int launch_composite_bwd_rays(int64_t n, int S, const float* raw, const float* z, const float* rays, const float* g_rgb,
                              const float* g_depth, const float* g_acc, const float* g_w, int accumulate, float* g_rays,
                              hipStream_t stream) {
    if (n <= 0) return 0;
    dispatch_G(S, [&](auto g) {
        constexpr int G = decltype(g)::value;
        hipLaunchKernelGGL(composite_bwd_rays_kernel<G>, ray_grid<G>(n), dim3(256), (size_t)(256 / G) * S * sizeof(float),
                           stream, n, S, raw, z, rays, g_rgb, g_depth, g_acc, g_w, accumulate, g_rays);
    });
    return check_launch("composite_bwd_rays");
}

int launch_sample_pdf(int64_t n, int nb, int ns, const float* bins, const float* weights, const float* u_lin, float* out,
                      hipStream_t stream) {
    if (n <= 0 || ns <= 0) return 0;
    const size_t lds = (size_t)4 * 2 * nb * sizeof(float);
    if (lds > 160 * 1024) { set_error("sample_pdf: %d bins exceed LDS", nb); return -1; }
    int64_t blocks = (n + 3) / 4;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(sample_pdf_kernel, dim3((unsigned)blocks), dim3(256), lds, stream, n, nb, ns, bins, weights, u_lin,
                       out);
    return check_launch("sample_pdf");
}

// ---------------------------------------------------------------------------------------
// One field for both passes (pi_GAN renders with coarse_model is fine_model, pi_GAN/modules.py:160-161; nerf with
// use_fine_model off, nerf/train_nerf.py:91,94): the fine pass of render_rays (render.py:143-144) evaluates the field at
// sort(cat(z_coarse, z_samples)) - and Nc of those Nc + Nf points are the very points the coarse pass evaluated, with the
// same field: identical inputs, identical outputs.  The renderer then evaluates the Nf NEW points only and puts the
// two sets of raw values into the sorted order with the positions the merge computed (`pos` of sample_fine_kernel:
// pos[e] = index in z_fine of input element e, e < Nc coarse, else sample e - Nc).  Generalises the Nf = 0 alias of
// SURVEY.md 8d C2; bit-identical to evaluating all Nc + Nf points because a point's value does not depend on which
// launch or lane computed it.
//   merge_raw:  raw_f[pos[e]] = e < Nc ? raw_c[e] : raw_s[e - Nc]
//   split_grad: the transpose, for the backward pass: g_c[e] (+)= g_f[pos[e]], g_s[i] = g_f[pos[Nc + i]]
// thread per (ray, element); float4 per point.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void merge_raw_kernel(int64_t n, int nc, int nf, const float4* __restrict__ raw_c,
                                                        const float4* __restrict__ raw_s, const int* __restrict__ pos,
                                                        float4* __restrict__ raw_f) {
    const int S = nc + nf;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * S) return;
    const int64_t ray = i / S;
    const int e = (int)(i - ray * S);
    raw_f[ray * S + pos[i]] = e < nc ? raw_c[ray * nc + e] : raw_s[ray * nf + (e - nc)];
}

__global__ __launch_bounds__(256) void split_grad_kernel(int64_t n, int nc, int nf, const float4* __restrict__ g_f,
                                                         const int* __restrict__ pos, float4* __restrict__ g_c,
                                                         int accumulate_coarse, float4* __restrict__ g_s) {
    const int S = nc + nf;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * S) return;
    const int64_t ray = i / S;
    const int e = (int)(i - ray * S);
    const float4 g = g_f[ray * S + pos[i]];
    if (e < nc) {
        float4* d = g_c + ray * nc + e;
        if (accumulate_coarse) { const float4 o = *d; *d = make_float4(o.x + g.x, o.y + g.y, o.z + g.z, o.w + g.w); }
        else *d = g;
    } else {
        g_s[ray * nf + (e - nc)] = g;
    }
}

int launch_merge_raw(int64_t n, int nc, int nf, const float* raw_c, const float* raw_s, const int* pos, float* raw_f,
                     hipStream_t stream) {
    const int64_t total = n * (nc + nf);
    if (total <= 0) return 0;
    hipLaunchKernelGGL(merge_raw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, n, nc, nf,
                       (const float4*)raw_c, (const float4*)raw_s, pos, (float4*)raw_f);
    return check_launch("merge_raw");
}

int launch_split_grad(int64_t n, int nc, int nf, const float* g_f, const int* pos, float* g_c, int accumulate_coarse,
                      float* g_s, hipStream_t stream) {
    const int64_t total = n * (nc + nf);
    if (total <= 0) return 0;
    hipLaunchKernelGGL(split_grad_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, n, nc, nf,
                       (const float4*)g_f, pos, (float4*)g_c, accumulate_coarse, (float4*)g_s);
    return check_launch("split_grad");
}

// one launch of either instance of sample_fine_kernel: lin = the z_lin table (or null), with kBounds the bounds [n,2]
template <bool kBounds>
static int launch_sample_fine_as(const char* what, int64_t n, float near_, float far_, int nc, int nf, const float* lin,
                                 const float* u_lin, const float* z_coarse, const float* weights, float* z_samples,
                                 float* z_fine, int* pos, hipStream_t stream) {
    if (n <= 0) return 0;
    const size_t lds = (size_t)4 * (2 * nc + 2 * (nc + nf)) * sizeof(float);
    if (lds > 64 * 1024) { set_error("%s: Nc=%d Nf=%d exceed LDS", what, nc, nf); return -1; }
    int64_t blocks = (n + 3) / 4;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(sample_fine_kernel<kBounds>, dim3((unsigned)blocks), dim3(256), lds, stream, n, near_, far_, nc, nf,
                       lin, u_lin, z_coarse, weights, z_samples, z_fine, pos);
    return check_launch(what);
}

int launch_sample_fine(int64_t n, float near_, float far_, int nc, int nf, const float* z_lin, const float* u_lin,
                       const float* z_coarse, const float* weights, float* z_samples, float* z_fine, int* pos,
                       hipStream_t stream) {
    return launch_sample_fine_as<false>("sample_fine", n, near_, far_, nc, nf, z_lin, u_lin, z_coarse, weights, z_samples,
                                        z_fine, pos, stream);
}

int launch_sample_fine_bounds(int64_t n, const float* bounds, int nc, int nf, const float* u_lin, const float* z_coarse,
                              const float* weights, float* z_samples, float* z_fine, int* pos, hipStream_t stream) {
    return launch_sample_fine_as<true>("sample_fine_bounds", n, 0.f, 0.f, nc, nf, bounds, u_lin, z_coarse, weights, z_samples,
                                       z_fine, pos, stream);
}

// ---------------------------------------------------------------------------------------
// out[0, count) = 0.f - and zero bits are zero ints: the clear of every buffer that launches behind it add to (g_rays of
// the occupancy backward) or count into (the live counts of the windowed coarse pass and of the deferred colour branch).
// A kernel, not hipMemsetAsync: captured into a graph, a memset of more than 12 bytes, or one that crosses a 16-byte
// line, cleared its bytes on the first replay only (tools/probes/graph_memset_probe.py, profiles/graph_memset_probe.log;
// DESIGN.md 4.8 "In a graph").  Eager calls never showed it.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void clear_floats_kernel(int64_t count, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < count) out[i] = 0.f;
}

int launch_clear_floats(int64_t count, float* out, hipStream_t stream) {
    if (count <= 0) return 0;
    hipLaunchKernelGGL(clear_floats_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, count, out);
    return check_launch("clear_floats");
}

}  // namespace mi
