// field_bwd_dw.hip - the weight-gradient engines of the field backward (gfx950), the host planner that batches their jobs,
// the scratch-size queries, and the orchestration of a whole backward pass: the chain (field_bwd_chain.hip, through the
// launcher pair of field_bwd.h), then every weight gradient of the kind's graph (field_kinds.h).  This is the unit a
// feature edits; the chain kernels are not compiled here.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "field_bwd.h"
#include "field_kinds_host.h"
#include "field_mlp_device.h"
#include "launchers.h"

#include <type_traits>

namespace mi {

// FiLM layer finishing for ONE image (group) g.  T[f][k] = sum_{p in g} dL/du[p][f] X[p][k] (tk = 256, or the 3
// raw-input columns), s[f] = sum_{p in g} dL/du[p][f].  Row f per workgroup, column k per thread:
//   dW[f][col0+k]  (+)= gamma[f] T[f][k]                       (+= for g > 0: images are summed in order)
//   d gamma_g[f]   (+)= sum_k W[f][col0+k] T[f][k]  (+ b[f] s[f] with the bias part: A = W x + b)
//   d beta_g[f]      = s[f];   db[f] (+)= gamma[f] s[f]        (bias part only)
constexpr int kMaxFinishJobs = kFilmDepthMax + 2;   // an image's FiLM layers (at most 13) + the dir columns of hidden_layer_rgb
struct FinishJob {
    const float* T; const float* s; const float* W; const float* b; const float* film_row;
    float* dW; float* db; float* dfilm_row;
    int tk, w_ld, col0, bias_part;
};
struct FinishBatch { FinishJob job[kMaxFinishJobs]; int first_group; };

// grid = (256 rows, jobs): every finishing job of one image in ONE launch (round 2: ten launches of 4.6 us per image,
// 320 per C4 step).  A job that adds to a d gamma another job of the same launch WRITES (hidden_layer_rgb's dir columns
// after its h columns: bias_part = 0) runs in the same workgroup right after it - see film_images_backward.
__global__ __launch_bounds__(256) void film_finish_kernel(FinishBatch fb) {
    __shared__ float red[4];
    const int f = blockIdx.x, k = threadIdx.x;
    const int first_group = fb.first_group;
    // blockIdx.y indexes the jobs with a bias part; a job without one (it ADDS to the d gamma row of the job before it
    // in the table) is chained behind its predecessor here, so the two never race
    int j = 0;
    for (int seen = -1; j < kMaxFinishJobs; ++j)
        if (fb.job[j].T && fb.job[j].bias_part && ++seen == (int)blockIdx.y) break;
    if (j >= kMaxFinishJobs) return;
    for (; j < kMaxFinishJobs && fb.job[j].T; ++j) {
        const FinishJob& q = fb.job[j];
        const float gamma = q.film_row[f];
        float dot = 0.f;
        if (k < q.tk) {
            const float t = q.T[f * q.tk + k];
            float* w = q.dW + (int64_t)f * q.w_ld + q.col0 + k;
            *w = first_group ? gamma * t : *w + gamma * t;
            dot = q.W[(int64_t)f * q.w_ld + q.col0 + k] * t;
        }
        for (int off = 32; off > 0; off >>= 1) dot += __shfl_xor(dot, off);
        __syncthreads();                                   // red[] of the previous job of this chain has been consumed
        if ((k & 63) == 0) red[k >> 6] = dot;
        __syncthreads();
        if (k == 0) {
            float dg = ((red[0] + red[1]) + red[2]) + red[3];
            if (q.bias_part) {
                dg += q.b[f] * q.s[f];
                q.dfilm_row[f] = dg;
                q.dfilm_row[256 + f] = q.s[f];
                q.db[f] = first_group ? gamma * q.s[f] : q.db[f] + gamma * q.s[f];
            } else {
                q.dfilm_row[f] += dg;
            }
        }
        if (j + 1 < kMaxFinishJobs && fb.job[j + 1].T && fb.job[j + 1].bias_part) break;     // the next job is another chain's head
    }
}

// =========================================================================================
// dW GEMM over points: dW[f][k] = sum_p dA[p][f] X[p][k].  Features sit on the MFMA lanes: lane i of wave-tile
// (wm, wk) owns dA features 128*wm + 4*i + c (c = the four 32-wide row blocks) and X features 32*CB*wk + CB*i + d,
// acc[c][d] (+)= A_c (x) B_d per point pair.  Workgroup = 4 waves = tiles (WM x WK) x k-split KS = 4 / (WM*WK).
// partial record (slab) = [TM][TK] row-major tile, then (with_bias) the TM column sums of dA.
// Rows are staged through LDS by DMA (buffer_load ... lds) rather than loaded per lane (the first version: 4 ms
// of a 60 ms step slower):
// a stage = 32 points = one contiguous run of rows of each operand ([point][feature] rows with lda == TM and
// ldx == TK, which holds for every job), double-buffered; the next stage's 1 KiB pieces are issued one per 8
// MFMAs during the first half of the current stage, so they have half a stage (>= 3 us) to land.  Rows past the
// slab's end read as zero (buffer bounds), so ragged slabs need no masking.  Operand fetch is one ds_read_b128
// (conflict-free: 16 consecutive lanes read 16 consecutive float4) per operand and point pair.
constexpr int kGemmStagePts = 32;

// Up to kMaxGemmJobs GEMMs of one tile shape in ONE launch (grid.y = job): every job contracts the same P points, so
// a training step's nine 256x256 weight gradients are one launch of 9 x slabs workgroups instead of nine launches
// of `slabs` - at the 1024-ray batch of nerf/train_nerf.py the step is launch-bound otherwise.
constexpr int kMaxGemmJobs = 12;
struct GemmBatch {
    const float* dA[kMaxGemmJobs];
    const float* X[kMaxGemmJobs];
    float* partial[kMaxGemmJobs];      // one record per slab of TM*TK (+ TM bias sums) floats
    int with_bias[kMaxGemmJobs];
};

// LDS floats one k-split wave parks for the merge (its 4 x CB accumulator blocks + the bias sums), and the dynamic LDS a
// launch needs: the two stage buffers, or the merge area of the (KS - 1) x TILES parked waves if that is larger.
constexpr int gemm_merge_wave_floats(int CB) { return (4 * CB * 16 + 4) * 64; }
// Stage buffers in the ring.  A 256x256 tile runs 256 MFMAs per wave and stage (6.9 us) on 64 KiB of rows: one stage in
// flight while the other is consumed hides the memory latency, and two buffers are all that fit.  The NARROW tiles run 16 -
// 128 MFMAs (0.4 - 3.4 us) on 20 - 48 KiB: with one stage in flight a CU has ~40 KiB outstanding against a loaded HBM latency
// of ~2 us - Little's law caps the chip at ~2.5 TB/s, which is what round 3 measured for them (2.0 - 2.5 TB/s of algorithmic
// bytes at 0.25 - 0.65 MFMA-busy) while they ask for 3.6 - 6 TB/s.  Their stages are small, so the ring holds one or two more.
template <int CB, int WM, int WK>
constexpr int gemm_ring() {
    constexpr size_t stage = (size_t)kGemmStagePts * (128 * WM + 32 * CB * WK) * sizeof(float);
    return stage >= 64 * 1024 ? 2 : (stage > 20 * 1024 ? 3 : 4);
}
template <int CB, int WM, int WK>
constexpr size_t gemm_lds_bytes() {
    constexpr int TILES = WM * WK, KS = 4 / TILES, TM = 128 * WM, TK = 32 * CB * WK;
    constexpr size_t stage = (size_t)gemm_ring<CB, WM, WK>() * kGemmStagePts * (TM + TK) * sizeof(float);
    constexpr size_t merge = (size_t)(KS - 1) * TILES * gemm_merge_wave_floats(CB) * sizeof(float);
    return stage > merge ? stage : merge;
}

// COUNTED: the rows and the slab length come from the device count (counted_slab_pts); a slab past the rows contracts nothing
// (its descriptors bound zero records, its ring reads zeros) and writes a zero record.
template <int CB, int WM, int WK, bool COUNTED = false>
__global__ __launch_bounds__(256, 1) void dw_gemm_kernel(GemmBatch jobs, std::conditional_t<COUNTED, CountedRows, int64_t> rows_in,
                                                         int slab_in) {
    int64_t P;
    int slab_pts;
    if constexpr (COUNTED) {
        P = counted_rows(rows_in.count, rows_in.capacity);
        slab_pts = counted_slab_pts(P, rows_in.n_slabs);
    } else {
        P = rows_in;
        slab_pts = slab_in;
    }
    const float* __restrict__ dA = jobs.dA[blockIdx.y];
    const float* __restrict__ X = jobs.X[blockIdx.y];
    float* __restrict__ partial = jobs.partial[blockIdx.y];
    const int with_bias = jobs.with_bias[blockIdx.y];
    constexpr int TILES = WM * WK, KS = 4 / TILES, TM = 128 * WM, TK = 32 * CB * WK, T = kGemmStagePts;
    constexpr int PA = T * TM / 256, PB = T * TK / 256;              // 1 KiB pieces per stage and operand
    constexpr int NPW = (PA + PB + 3) / 4;                           // pieces per wave and stage
    constexpr int STEPS = (T / 2) / KS;                              // point pairs per wave and stage
    constexpr int PPS = (NPW + STEPS / 2 - 1) / (STEPS / 2);         // pieces issued per step in the first half
    constexpr int STAGE = T * (TM + TK);                             // floats per stage buffer
    typedef float bvec __attribute__((ext_vector_type(CB)));
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = lane & 31, h = lane >> 5;
    const int tile = wave % TILES, ks = wave / TILES;
    const int wm = tile / WK, wk = tile % WK;
    const int64_t p0 = (int64_t)blockIdx.x * slab_pts;
    int64_t p1 = p0 + slab_pts < P ? p0 + slab_pts : P;
    if constexpr (COUNTED) p1 = p1 < p0 ? p0 : p1;                   // an empty slab: zero records, zero stages
    const int n_stages = (int)((p1 - p0 + T - 1) / T);
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)(dA + p0 * TM), 0, (int)((p1 - p0) * TM * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)(X + p0 * TK), 0, (int)((p1 - p0) * TK * 4), 0x00020000);
    // piece q (0..PA+PB-1) of stage st into buffer b; wave w owns pieces w, w+4, ...
    const auto issue = [&](int st, int b, int k) {
        const int q = wave + 4 * k;
        if (q < PA)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (MI_LDS void*)(smem + b * STAGE + q * 256), 16, lane * 16,
                                                     st * (T * TM * 4) + q * 1024, 0, 0);
        else if (q < PA + PB)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, (MI_LDS void*)(smem + b * STAGE + T * TM + (q - PA) * 256), 16,
                                                     lane * 16, st * (T * TK * 4) + (q - PA) * 1024, 0, 0);
    };

    f32x16 acc[4][CB];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int d = 0; d < CB; ++d)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[c][d][r] = 0.f;
    f32x4 bsum = {0.f, 0.f, 0.f, 0.f};

    // Ring of NB stage buffers: stages st+1 .. st+NB-2 are in flight while stage st is consumed, and stage st+NB-1 is
    // issued during it (into the buffer stage st-1 just left).  Every wave issues exactly NPW pieces per stage, ALWAYS -
    // stages past the slab's end read zeros through the buffer bounds and are never consumed - so "stage st has landed" is
    // `s_waitcnt vmcnt((NB - 2) * NPW)`: the wave's vector-memory operations complete in order and nothing else is issued
    // in the loop.
    constexpr int NB = gemm_ring<CB, WM, WK>();
    static_assert((PA + PB) % 4 == 0, "every wave must issue the same number of pieces per stage (the vmcnt arithmetic)");
    static_assert((NB - 2) * NPW < 64, "vmcnt is a 6-bit counter");
#pragma unroll
    for (int sp = 0; sp < NB - 1; ++sp)
#pragma unroll
        for (int k = 0; k < NPW; ++k) issue(sp, sp, k);
    int b = 0;
    for (int st = 0; st < n_stages; ++st) {
        // stage st has landed in every wave's view: own pieces by the count, the others' by the barrier
        asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"((NB - 2) * NPW) : "memory");
        const int bn = b == 0 ? NB - 1 : b - 1;                      // the buffer stage st - 1 used = (st + NB - 1) % NB
        // this wave's first point pair of the stage; step sidx reads rows 2 KS sidx further on (an immediate offset)
        const float* As = smem + b * STAGE + 128 * wm + 4 * i + (2 * ks + h) * TM;
        const float* Bs = smem + b * STAGE + T * TM + 32 * CB * wk + CB * i + (2 * ks + h) * TK;
        // Operands one step ahead: the reads of step s + 1 are issued at the top of step s and pinned there, so their LDS
        // latency runs under the 4 CB MFMAs of step s.  (Left to the scheduler, the A operand of a step was read three MFMAs
        // before the step began with an s_waitcnt lgkmcnt(0) right behind it - the matrix pipe drained at every step: the
        // ISA of round 2's kernel, tools/isa_stats.py.)  Only the first step of a stage waits for LDS.
        f32x4 av = *reinterpret_cast<const f32x4*>(As);
        bvec bv = *reinterpret_cast<const bvec*>(Bs);
        static_for<STEPS>([&](auto sc) {
            constexpr int sidx = decltype(sc)::value;
            f32x4 av_n = av;
            bvec bv_n = bv;
            if constexpr (sidx + 1 < STEPS) {
                av_n = *reinterpret_cast<const f32x4*>(As + 2 * KS * (sidx + 1) * TM);
                bv_n = *reinterpret_cast<const bvec*>(Bs + 2 * KS * (sidx + 1) * TK);
                __builtin_amdgcn_sched_barrier(0);
            }
            bsum += av;
            static_for<4>([&](auto cc) {
                constexpr int c = decltype(cc)::value;
#pragma unroll
                for (int d = 0; d < CB; ++d)
                    acc[c][d] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[c], bv[d], acc[c][d], 0, 0, 0);
                // first half of the stage: up to PPS pieces of the next stage per step, one after each group of CB MFMAs
                constexpr int slot = sidx * PPS + c;
                if constexpr (sidx < STEPS / 2 && c < PPS && slot < NPW) {
                    __builtin_amdgcn_sched_barrier(0);
                    issue(st + NB - 1, bn, slot);
                    __builtin_amdgcn_sched_barrier(0);
                }
            });
            av = av_n;
            bv = bv_n;
        });
        b = b + 1 == NB ? 0 : b + 1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                 // the zero stages issued past the slab's end
    // The k-split waves of a workgroup (KS = 2 or 4 for the narrow tiles) hold partial sums of the SAME tile: they are
    // added here, through the stage buffers, in k order - one record per slab instead of KS (the narrow GEMMs of a
    // NeRF step wrote and re-read 2-4x the partial bytes of the wide ones for a fraction of their work).
    if constexpr (KS > 1) {
        constexpr int WF = gemm_merge_wave_floats(CB);
        __syncthreads();                                             // every wave has left the stage buffers
        if (ks > 0) {
            float* mine = smem + ((ks - 1) * TILES + tile) * WF + lane;
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int d = 0; d < CB; ++d)
#pragma unroll
                    for (int r = 0; r < 16; ++r) mine[((c * CB + d) * 16 + r) * 64] = acc[c][d][r];
#pragma unroll
            for (int q = 0; q < 4; ++q) mine[(4 * CB * 16 + q) * 64] = bsum[q];
        }
        __syncthreads();
        if (ks > 0) return;
#pragma unroll
        for (int k = 1; k < KS; ++k) {
            const float* o = smem + ((k - 1) * TILES + tile) * WF + lane;
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int d = 0; d < CB; ++d)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[c][d][r] += o[((c * CB + d) * 16 + r) * 64];
#pragma unroll
            for (int q = 0; q < 4; ++q) bsum[q] += o[(4 * CB * 16 + q) * 64];
        }
    }
    // write the partial tile: D[row i'][col j] on lane (j, h), reg r: i' = (r&3) + 8*(r>>2) + 4*h
    float* out = partial + (int64_t)blockIdx.x * (TM * TK + (with_bias ? TM : 0));
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ip = (r & 3) + 8 * (r >> 2) + 4 * h;
            bvec v;
#pragma unroll
            for (int d = 0; d < CB; ++d) v[d] = acc[c][d][r];
            *reinterpret_cast<bvec*>(out + (int64_t)(128 * wm + 4 * ip + c) * TK + 32 * CB * wk + CB * i) = v;
        }
    if (with_bias && wk == 0) {
        bsum.x += __shfl_xor(bsum.x, 32); bsum.y += __shfl_xor(bsum.y, 32);
        bsum.z += __shfl_xor(bsum.z, 32); bsum.w += __shfl_xor(bsum.w, 32);
        if (h == 0) *reinterpret_cast<f32x4*>(out + TM * TK + 128 * wm + 4 * i) = bsum;
    }
}

// Thin gradients: out[c][f] = sum_p S[p][c0+c] * H[p][f] for c < nc <= 3, f < F <= 256, plus sum_p S[p][c0+c], plus - in
// the record's fourth row, free once the rows are being read - the column sums sum_p H[p][f] (the bias gradient of a
// layer whose weights are all K = 3 columns).
//   heads:        S = head pre-activation grads [P,4], H = the head's input  -> dW_head[c][f], db_head[c]
//   K = 3 inputs: S = xin [P,8] (xyz | dir),           H = dA of the layer   -> dW[f][col0 + c]
// grid = (point slabs, jobs), block = 256 threads = features; partial[slab][4][256], bias_partial[slab][4] per job.
constexpr int kMaxThinJobs = 6;
struct ThinBatch {
    const float* S[kMaxThinJobs]; const float* H[kMaxThinJobs];
    float* partial[kMaxThinJobs]; float* bias_partial[kMaxThinJobs];
    int lds_[kMaxThinJobs], c0[kMaxThinJobs], nc[kMaxThinJobs], ldh[kMaxThinJobs], F[kMaxThinJobs];
};
template <bool COUNTED = false>
__global__ __launch_bounds__(256) void thin_grad_kernel(ThinBatch tb, std::conditional_t<COUNTED, CountedRows, int64_t> rows_in, int slab_in) {
    int64_t P;
    int slab_pts;
    if constexpr (COUNTED) {                    // as in dw_gemm_kernel; an empty slab's loops do not run: a zero record
        P = counted_rows(rows_in.count, rows_in.capacity);
        slab_pts = counted_slab_pts(P, rows_in.n_slabs);
    } else {
        P = rows_in;
        slab_pts = slab_in;
    }
    const int job = blockIdx.y;
    const float* __restrict__ S = tb.S[job];
    const float* __restrict__ H = tb.H[job];
    float* __restrict__ partial = tb.partial[job];
    float* __restrict__ bias_partial = tb.bias_partial[job];
    const int lds_ = tb.lds_[job], c0 = tb.c0[job], nc = tb.nc[job], ldh = tb.ldh[job], F = tb.F[job];
    // wave w takes points p0 + w, p0 + w + 4, ...; lane l the features 4l..4l+3 (float4 rows, 4 points in flight);
    // the four waves' sums are added in wave order at the end, so the result does not depend on timing
    __shared__ float red[4][4][256];
    __shared__ float bred[4][4];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t p0 = (int64_t)blockIdx.x * slab_pts;
    const int64_t p1 = p0 + slab_pts < P ? p0 + slab_pts : P;
    const bool live = 4 * lane < F;
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0, a3 = a0;
    float b0 = 0.f, b1 = 0.f, b2 = 0.f;
    const auto row = [&](int64_t p) {
        return live ? *reinterpret_cast<const f32x4*>(H + p * ldh + 4 * lane) : f32x4{0.f, 0.f, 0.f, 0.f};
    };
    const auto fma_row = [&](int64_t p, const f32x4& hv) {
        const float* sp = S + p * lds_ + c0;
        const float s0 = sp[0], s1 = nc > 1 ? sp[1] : 0.f, s2 = nc > 2 ? sp[2] : 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            a0[q] = fmaf(s0, hv[q], a0[q]); a1[q] = fmaf(s1, hv[q], a1[q]); a2[q] = fmaf(s2, hv[q], a2[q]);
        }
        a3 += hv;
        b0 += s0; b1 += s1; b2 += s2;
    };
    // eight rows in flight per wave (and four workgroups per CU: BwdBatcher::flush_thin): this kernel is a stream over
    // P x 1 KiB rows, and with four rows per wave and one workgroup per CU only 16 KiB per CU were in flight - 2.9 TB/s
    int64_t p = p0 + w;
    for (; p + 28 < p1; p += 32) {
        const f32x4 h0 = row(p), h1 = row(p + 4), h2 = row(p + 8), h3 = row(p + 12);
        const f32x4 h4 = row(p + 16), h5 = row(p + 20), h6 = row(p + 24), h7 = row(p + 28);
        fma_row(p, h0); fma_row(p + 4, h1); fma_row(p + 8, h2); fma_row(p + 12, h3);
        fma_row(p + 16, h4); fma_row(p + 20, h5); fma_row(p + 24, h6); fma_row(p + 28, h7);
    }
    for (; p < p1; p += 4) fma_row(p, row(p));
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        red[w][0][4 * lane + q] = a0[q]; red[w][1][4 * lane + q] = a1[q]; red[w][2][4 * lane + q] = a2[q];
        red[w][3][4 * lane + q] = a3[q];
    }
    if (lane == 0) { bred[w][0] = b0; bred[w][1] = b1; bred[w][2] = b2; }
    __syncthreads();
    const int f = threadIdx.x;
    float* out = partial + (int64_t)blockIdx.x * 4 * 256;
#pragma unroll
    for (int c = 0; c < 4; ++c) out[c * 256 + f] = ((red[0][c][f] + red[1][c][f]) + red[2][c][f]) + red[3][c][f];
    if (f < 4) {
        float* bo = bias_partial + (int64_t)blockIdx.x * 4;
        bo[f] = f < 3 ? ((bred[0][f] + bred[1][f]) + bred[2][f]) + bred[3][f] : 0.f;
    }
}

// Every cross-slab reduction of a backward pass in ONE launch (grid.y = job), fixed order, deterministic.  A job sums
// n records of `rec` floats element-wise; element idx < TM*TK is tile entry (row, col) = (idx / TK, idx % TK), the
// tail (when bias_dst) the TM bias sums.  Placement: dst[row*ld + col0 + col], or transposed (K = 3 weight columns:
// record [c][f] -> dst[f*ld + col0 + c]).
constexpr int kMaxReduceJobs = 24;
struct ReduceJob {
    const float* src;
    float* dst;
    float* bias_dst;
    int n, rec, TM, TK, ld, col0, rows_valid, cols_valid, transposed;
    int row0 = 0;               // first record row the job places (rows below it belong to another job over the same records)
};
struct ReduceBatch { ReduceJob job[kMaxReduceJobs]; };

__global__ __launch_bounds__(256) void reduce_jobs_kernel(ReduceBatch rb) {
    // Block = 32 float4 entries x 8 k-lanes: lane g sums records g, g+8, g+16, ... (four 16-byte loads in flight), the
    // eight lane sums are added in lane order through LDS - a fixed order whatever the timing.  A job's critical path
    // is n/8 dependent-latency loads instead of n: the 128 x 256 GEMM of a NeRF's dir layer leaves 512 records
    // (256 slabs x 2 k-splits), and with one thread walking all of them the whole launch waited 130 us for it.
    __shared__ f32x4 part[8][32];
    const ReduceJob& j = rb.job[blockIdx.y];
    const int x = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int idx = (blockIdx.x * 32 + x) * 4;
    const bool live = idx < j.rec;
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0, s2 = s0, s3 = s0;
    if (live) {
        const f32x4* p = reinterpret_cast<const f32x4*>(j.src + idx);
        const int64_t stride4 = j.rec / 4;
        int k = g;
        for (; k + 24 < j.n; k += 32) {
            s0 += p[(int64_t)k * stride4]; s1 += p[(int64_t)(k + 8) * stride4];
            s2 += p[(int64_t)(k + 16) * stride4]; s3 += p[(int64_t)(k + 24) * stride4];
        }
        for (; k < j.n; k += 8) s0 += p[(int64_t)k * stride4];
    }
    part[g][x] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (g != 0 || !live) return;
    f32x4 s = part[0][x];
#pragma unroll
    for (int t = 1; t < 8; ++t) s += part[t][x];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = idx + q;
        const bool is_bias = e >= j.TM * j.TK;
        const int row = is_bias ? e - j.TM * j.TK : e / j.TK, col = is_bias ? 0 : e % j.TK;
        if (row >= j.rows_valid || (!is_bias && (col >= j.cols_valid || row < j.row0)) || (is_bias && !j.bias_dst)) continue;
        if (is_bias) j.bias_dst[row] = s[q];
        else if (j.transposed) j.dst[(int64_t)col * j.ld + j.col0 + row] = s[q];
        else j.dst[(int64_t)(row - j.row0) * j.ld + j.col0 + col] = s[q];
    }
}

// ---- host orchestration ---------------------------------------------------------------------
// FiLM scratch: one image's T_l (256x256) and column sums s_l (256) per 256-wide layer, its raw-input columns (256x3, padded)
constexpr int64_t kFilmLayerScratch = 256 * 256 + 256;       // T_l and s_l of one 256-wide FiLM layer
// the L 256-wide FiLM layers of depth L, two K = 3 blocks, s_0 (film_images_backward)
int64_t film_partial_floats_kind(int kind, int64_t /*n_groups*/, int64_t /*points_per_group*/) {
    return is_film(kind) ? film_depth(kind) * kFilmLayerScratch + 2 * 256 * 4 + 256 : 0;
}
// the query without a kind is the reference's depth, kinds 2 / 3
int64_t film_partial_floats(int64_t n_groups, int64_t points_per_group) {
    return film_partial_floats_kind(MI_FIELD_FILM_SIREN_NERF, n_groups, points_per_group);
}

// The planner's worst case for one FiLM image of depth L of at most P points: L GEMM jobs of at most ceil(256 / L) slabs
// each, two thin jobs (or the two head jobs over all images).
static int64_t film_image_partial_floats(int L, int64_t P) {
    const int64_t slabs256 = (P + 255) / 256 > 0 ? (P + 255) / 256 : 1;          // BwdBatcher::slabs_for never exceeds this
    const int64_t cap = (256 + L - 1) / L;
    return L * (slabs256 < cap ? slabs256 : cap) * kFilmLayerScratch + 2 * (slabs256 < 512 ? slabs256 : 512) * 1280 + 4096;
}

static int64_t batched_partial_floats(int kind, int64_t P);
int64_t bwd_partial_floats(int64_t P) {
    // FiLM kinds: one image at a time, at the reference's depth (eight jobs of at most 32 slabs): an upper bound for any
    // image of at most P points.  launch_field_backward checks every pass's real plan against this figure (through
    // bwd_partial_floats_kind) before it launches anything.
    int64_t most = film_image_partial_floats(8, P);
    for (int kind = 0; kind < MI_FIELD_KINDS; ++kind) {                           // the others: every job of the pass at once
        if (kFieldKinds[kind].film) continue;
        const int64_t n = batched_partial_floats(kind, P);
        if (n > most) most = n;
    }
    return most;
}
// ... of any kind.  A FiLM image of depth L runs L GEMM jobs of at most ceil(256 / L) slabs each (BwdBatcher::slabs_for):
// 256 job-slabs at depths 4 and 8, but 260 / 258 / 259 at depths 5 / 6 / 7 and up to 264 (depth 12) above 8, so the figure
// above, written for eight jobs of 32 slabs, does not state every depth's plan.  At depths 5 to 7 it is still large enough:
// the extra job-slabs (at most 4 x 65 792 floats) start at 9 217 points, where the NeRF plan in its maximum is already more
// than a million floats above the FiLM term (tests/test_cabi_train_sizes.py replays the planner against this query for
// every depth).  This one is the planner's worst case for the depth itself, never less than the figure above.
int64_t bwd_partial_floats_kind(int kind, int64_t P) {
    const int64_t base = bwd_partial_floats(P);
    const int L = film_depth(kind);
    const int64_t film = L ? film_image_partial_floats(L, P) : 0;
    return film > base ? film : base;
}


// ---- batched orchestration (NeRF, TinyNeRF, SirenNeRF) -----------------------------------------------------------
// A backward pass is: the chain kernel, then every weight-gradient GEMM of one tile shape in ONE launch (grid.y =
// job), the thin (1-/3-row) gradients in one launch, and ONE reduction launch that sums every job's slab partials
// into the gradient tensors - 8 launches for a NeRF (it was 41: at the 1024-ray batch of nerf/train_nerf.py the step
// is launch-bound).  With several jobs per launch a job needs fewer slabs to fill the chip (slabs x jobs ~ 2 per
// CU), so the partial tiles written and re-read shrink by the same factor.
struct BwdBatcher {
    int64_t P;
    float* partial;            // scratch base (null: plan only - used to size the scratch)
    int64_t used = 0;          // floats of scratch handed out
    hipStream_t stream;
    const int* count = nullptr;   // a counted pass: rows [0, *count) of P (the capacity the plan is made from)
    struct Group { GemmBatch b{}; int n = 0; ReduceJob red[kMaxGemmJobs]; } g422, g221, g412, g111;
    ThinBatch thin{};
    int n_thin = 0;
    // the reductions of the thin jobs' records: thin job `thin`'s partial records, or (bias) its bias records
    struct ThinReduce { ReduceJob job; int thin; bool bias; } thin_red[3 * kMaxThinJobs];
    int n_thin_red = 0;
    ReduceBatch all{};
    int n_red = 0, max_rec = 0;

    static int slabs_for(int64_t P, int njobs, int per_cu = 1) {
        // one workgroup per CU over the whole launch: the workgroups of a launch do equal work, so a single wave of
        // them has no tail, and fewer slabs mean fewer partial tiles to write and to sum.  (per_cu = 4 for the thin
        // gradients: a 256-thread streaming kernel with no LDS to speak of needs several workgroups per CU to keep
        // enough loads in flight, and its records are 4 KiB, not 256 KiB.)
        int64_t s = (256 * per_cu + njobs - 1) / njobs;
        if (s > 256 * per_cu) s = 256 * per_cu;
        const int64_t most = (P + 255) / 256;              // slabs of at least 256 points
        if (s > most) s = most;
        return (int)(s < 1 ? 1 : s);
    }
    static int slab_pts_for(int64_t P, int slabs) { return (int)(((P + slabs - 1) / slabs + 31) / 32 * 32); }
    // The slabs of one launch of njobs jobs: their length in points and how many cover P (one record per slab and job).
    struct SlabPlan { int slab, n_slabs; };
    SlabPlan plan_slabs(int njobs, int per_cu = 1) const {
        const int slab = slab_pts_for(P, slabs_for(P, njobs, per_cu));
        return {slab, (int)((P + slab - 1) / slab)};
    }
    // One launch of a kernel pair over grid (slabs, jobs): the plain instance over P points in slabs of sp.slab, or - a
    // counted pass - the counted instance, which cuts the rows the device count gives into the plan's n_slabs.
    template <class Batch>
    int launch_slabs(void (*plain)(Batch, int64_t, int), void (*counted)(Batch, CountedRows, int), const SlabPlan& sp, int njobs,
                     size_t lds, const Batch& batch, const char* what) {
        if (count)
            hipLaunchKernelGGL(counted, dim3(sp.n_slabs, njobs), dim3(256), lds, stream, batch, CountedRows{count, P, sp.n_slabs}, 0);
        else
            hipLaunchKernelGGL(plain, dim3(sp.n_slabs, njobs), dim3(256), lds, stream, batch, P, sp.slab);
        return check_launch(what);
    }

    float* take(int64_t floats) {
        float* p = partial ? partial + used : nullptr;
        used += (floats + 255) / 256 * 256;
        return p;
    }
    void add_reduce(const ReduceJob& j) {
        all.job[n_red++] = j;
        if (j.rec > max_rec) max_rec = j.rec;
    }
    // dW[M rows][w_ld] at column w_col0 (+ bias gradient gb) = dA^T X over the P points
    template <int CB, int WM, int WK>
    void gemm(Group& g, const float* dA, const float* X, float* gw, int w_ld, int w_col0, int rows_valid, int cols_valid,
              float* gb) {
        constexpr int TM = 128 * WM, TK = 32 * CB * WK;
        g.b.dA[g.n] = dA; g.b.X[g.n] = X; g.b.with_bias[g.n] = gb ? 1 : 0;
        g.red[g.n] = ReduceJob{nullptr, gw, gb, 0, TM * TK + (gb ? TM : 0), TM, TK, w_ld, w_col0, rows_valid, cols_valid, 0};
        ++g.n;
    }
    template <int CB, int WM, int WK>
    int flush(Group& g) {
        if (!g.n) return 0;
        const SlabPlan sp = plan_slabs(g.n);
        for (int i = 0; i < g.n; ++i) {
            g.red[i].n = sp.n_slabs;                          // one record per slab (k-split waves merge in the kernel)
            g.b.partial[i] = take((int64_t)g.red[i].n * g.red[i].rec);
            g.red[i].src = g.b.partial[i];
            add_reduce(g.red[i]);
        }
        if (!partial) return 0;
        constexpr size_t lds = gemm_lds_bytes<CB, WM, WK>();
        static_assert(lds <= 160 * 1024, "dw_gemm_kernel: this tile shape needs more LDS than a CU has");
        static PerDeviceOnce attr_once;                                               // one per template instance
        const int arc = attr_once.run([&]() {
            for (const void* f : {(const void*)dw_gemm_kernel<CB, WM, WK>, (const void*)dw_gemm_kernel<CB, WM, WK, true>})
                if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
                    set_error("hipFuncSetAttribute(dw_gemm) failed"); return -2;
                }
            return 0;
        });
        if (arc) return arc;
        return launch_slabs(dw_gemm_kernel<CB, WM, WK>, dw_gemm_kernel<CB, WM, WK, true>, sp, g.n, lds, g.b, "dw_gemm (batched)");
    }
    // out[c][f] = sum_p S[p][c0+c] H[p][f]: heads (dst [nc][F], bias gb[nc]) or K = 3 weight columns (transposed into
    // dst[f*ld + col0 + c], no bias)
    // colsum_dst: also dst[f] = sum_p H[p][f] (the record's fourth row)
    void thin_job(const float* S, int lds_, int c0, int nc, const float* H, int ldh, int F, float* dst, int ld, int col0,
                  bool transposed, float* gb, float* colsum_dst = nullptr) {
        const int i = n_thin++;
        thin.S[i] = S; thin.lds_[i] = lds_; thin.c0[i] = c0; thin.nc[i] = nc; thin.H[i] = H; thin.ldh[i] = ldh; thin.F[i] = F;
        // record [4][256]: row c, col f
        thin_red[n_thin_red++] = {transposed ? ReduceJob{nullptr, dst, nullptr, 0, 1024, 4, 256, ld, col0, nc, F, 1}
                                             : ReduceJob{nullptr, dst, nullptr, 0, 1024, 4, 256, F, 0, nc, F, 0}, i, false};
        if (gb) thin_red[n_thin_red++] = {ReduceJob{nullptr, gb, nullptr, 0, 4, 1, 4, 4, 0, 1, nc, 0}, i, true};
        if (colsum_dst) thin_red[n_thin_red++] = {ReduceJob{nullptr, colsum_dst, nullptr, 0, 1024, 4, 256, 256, 0, 4, F, 0, 3}, i, false};
    }
    // The job of one block of a kind's graph (field_kinds.h) into dst[..][ld] at column col0, the bias gradient into
    // bias_dst (null: none).  Engine and tile follow from the block's shape: a head's 1 or 3 rows are a thin job, the 3 raw
    // input columns a transposed one (its bias: the record's column sums), everything else the GEMM of its row widths.
    int add(const GraphBlock& q, float* dst, int ld, int col0, float* bias_dst) {
        if (q.head) thin_job(q.dA, q.da_ld, q.da_c0, q.rows, q.X, q.x_ld, q.cols, dst, ld, col0, false, bias_dst);
        else if (q.cls == SRC_XIN) thin_job(q.X, q.x_ld, q.x_c0, q.cols, q.dA, q.da_ld, q.rows, dst, ld, col0, true, nullptr, bias_dst);
        else if (q.da_ld == 256 && q.x_ld == 256) gemm<4, 2, 2>(g422, q.dA, q.X, dst, ld, col0, q.rows, q.cols, bias_dst);
        else if (q.da_ld == 256 && q.x_ld == 64) gemm<2, 2, 1>(g221, q.dA, q.X, dst, ld, col0, q.rows, q.cols, bias_dst);
        else if (q.da_ld == 128 && q.x_ld == 256) gemm<4, 1, 2>(g412, q.dA, q.X, dst, ld, col0, q.rows, q.cols, bias_dst);
        else if (q.da_ld == 128 && q.x_ld == 32) gemm<1, 1, 1>(g111, q.dA, q.X, dst, ld, col0, q.rows, q.cols, bias_dst);
        else { set_error("no dW engine for a %d x %d block (layer %d)", q.da_ld, q.x_ld, q.layer); return -1; }
        return 0;
    }
    // every launch of the pass: the four GEMM groups, the thin jobs, the reduction
    int flush_all() {
        int rc;
        if ((rc = flush<4, 2, 2>(g422))) return rc;
        if ((rc = flush<2, 2, 1>(g221))) return rc;
        if ((rc = flush<4, 1, 2>(g412))) return rc;
        if ((rc = flush<1, 1, 1>(g111))) return rc;
        if ((rc = flush_thin())) return rc;
        return reduce_all();
    }
    int flush_thin() {
        if (!n_thin) return 0;
        const SlabPlan sp = plan_slabs(n_thin, 4);
        for (int i = 0; i < n_thin; ++i) {
            thin.partial[i] = take((int64_t)sp.n_slabs * 1024);
            thin.bias_partial[i] = take((int64_t)sp.n_slabs * 4);
        }
        for (int k = 0; k < n_thin_red; ++k) {
            ReduceJob j = thin_red[k].job;
            j.n = sp.n_slabs;
            j.src = thin_red[k].bias ? thin.bias_partial[thin_red[k].thin] : thin.partial[thin_red[k].thin];
            add_reduce(j);
        }
        if (!partial) return 0;
        return launch_slabs(thin_grad_kernel<false>, thin_grad_kernel<true>, sp, n_thin, 0, thin, "thin_grad (batched)");
    }
    int reduce_all() {
        if (!partial || !n_red) return 0;
        hipLaunchKernelGGL(reduce_jobs_kernel, dim3((max_rec / 4 + 31) / 32, n_red), dim3(256), 0, stream, all);
        return check_launch("reduce_jobs");
    }
};
static_assert(kFilmDepthMax <= kMaxGemmJobs && kFilmDepthMax + 6 <= kMaxReduceJobs,
              "an image's FiLM layers are one GEMM batch and, with the thin jobs, one reduction batch");

// Visits the blocks of K's graph that `want` accepts, in for_each_block's order, until `visit` returns non-zero: that value.
template <class Want, class Visit>
static int walk_blocks(const FieldKind& K, const float* acts, const float* grads, int64_t P, int64_t p0, Want&& want, Visit&& visit) {
    int rc = 0;
    for_each_block(K, acts, grads, P, p0, [&](const GraphBlock& q) {
        if (!rc && want(q)) rc = visit(q);
    });
    return rc;
}
static bool any_block(const GraphBlock&) { return true; }
static bool head_block(const GraphBlock& q) { return q.head; }
static bool layer_block(const GraphBlock& q) { return !q.head; }

// One pass of a batcher: the job of every wanted block, rows from point p0 of the P the buffers hold, into the destination
// `to` gives it (its bias gradient only where the block carries the bias), then every launch.  b.partial == nullptr: plan
// only (b.used = scratch floats needed).
struct BlockDst { float* dst; int ld, col0; float* bias; };
template <class Want, class To>
static int batch_blocks(BwdBatcher& b, const FieldKind& K, const float* acts, const float* grads, int64_t P, int64_t p0, Want&& want,
                        To&& to) {
    const int rc = walk_blocks(K, acts, grads, P, p0, want, [&](const GraphBlock& q) {
        const BlockDst d = to(q);
        return b.add(q, d.dst, d.ld, d.col0, q.bias ? d.bias : nullptr);
    });
    return rc ? rc : b.flush_all();
}
// ... into the gradient tensors gp: the whole pass of a non-FiLM kind (any_block), the heads of a FiLM kind (head_block)
template <class Want>
static int batched_backward(const FieldKind& K, BwdBatcher& b, const float* acts, const float* grads, float* const* gp, Want&& want) {
    return batch_blocks(b, K, acts, grads, b.P, 0, want, [&](const GraphBlock& q) {
        return BlockDst{gp[2 * q.layer], q.w_ld, q.w_col0, gp[2 * q.layer + 1]};
    });
}

// A pass's job list is run twice: first as a plan (no scratch, nothing launched) whose scratch need is checked against
// what mi_field_bwd_partial_floats(P) told the caller to allocate - a planning / execution mismatch would otherwise be an
// out-of-bounds write by the GEMMs - then for real over `pts` points.  check = false skips the plan (a pass already
// checked for the same shape).
template <class Jobs>
static int plan_then_run(int kind, int64_t pts, int64_t P, float* partial, hipStream_t stream, const Jobs& jobs, bool check = true,
                         const int* count = nullptr) {
    if (check) {
        BwdBatcher plan{pts, nullptr, 0, stream};
        (void)jobs(plan);
        const int64_t limit = bwd_partial_floats_kind(kind, P);
        if (plan.used > limit) {
            set_error("backward scratch plan (%lld floats) exceeds mi_field_bwd_partial_floats (%lld)", (long long)plan.used,
                      (long long)limit);
            return -1;
        }
    }
    BwdBatcher run{pts, partial, 0, stream, count};
    return jobs(run);
}

// The non-head layers of a FiLM kind, image by image (fixed order, so the sums over images are deterministic): T_g, s_g of
// every block of a FiLM layer - the 256 x 256 GEMMs of an image are ONE launch (grid.y = layer, a job needs only 32 slabs to
// give every CU a workgroup, so 8x fewer partial tiles are written and re-read than with a launch per layer), the K = 3
// blocks one thin launch, one reduction launch for all of them - then per block (film_finish_kernel)
// dW += gamma_g (.) T_g, db += gamma_g (.) s_g, d gamma_g = <W, T_g> + b (.) s_g, d beta_g = s_g.
static int film_images_backward(int kind, const float* acts, const float* grads, int64_t n_groups, int64_t ppg, const float* film,
                                float* film_partial, float* grad_film, float* partial, float* const* gp,
                                const float* const* params, hipStream_t stream) {
    const FieldKind& K = field_kind(kind);
    const int64_t P = n_groups * ppg;
    const int L = film_depth(kind), n_film = L + 1;      // hidden_layers; rows of an image's FiLM table
    // FiLM scratch of the current image: T_l [256][256] + s_l [256] for the L 256-wide FiLM layers (eight at the reference's
    // depth), the K = 3 blocks of layer 0 (xyz) and of layer L (dir) as [256][3] (padded to 4), s_0 [256]
    const auto Tl = [&](int l) { return film_partial + (int64_t)(l - 1) * kFilmLayerScratch; };
    float* const T3 = film_partial + (int64_t)L * kFilmLayerScratch;
    float* const s0 = T3 + 2 * 256 * 4;
    const auto T = [&](const GraphBlock& q) { return q.cls == SRC_XIN ? T3 + (q.da_region ? 256 * 4 : 0) : Tl(q.da_region); };
    const auto s = [&](const GraphBlock& q) { return q.da_region ? Tl(q.da_region) + 256 * 256 : s0; };
    for (int64_t g = 0; g < n_groups; ++g) {
        const float* frow = film + (g * n_film) * kFilmRow;
        float* dfrow = grad_film + (g * n_film) * kFilmRow;
        const auto jobs = [&](BwdBatcher& bb) {
            return batch_blocks(bb, K, acts, grads, P, g * ppg, layer_block, [&](const GraphBlock& q) { return BlockDst{T(q), q.cols, 0, s(q)}; });
        };
        if (const int rc = plan_then_run(kind, ppg, P, partial, stream, jobs, g == 0)) return rc;   // the plan: first image only
        // a block without the bias part (hidden_layer_rgb's dir columns) is chained behind its layer's job before it
        FinishBatch fb{};
        int n_fin = 0, n_chains = 0;
        fb.first_group = g == 0;
        (void)walk_blocks(K, acts, grads, P, g * ppg, layer_block, [&](const GraphBlock& q) {
            fb.job[n_fin++] = FinishJob{T(q), s(q), params[2 * q.layer], params[2 * q.layer + 1], frow + q.da_region * kFilmRow,
                                        gp[2 * q.layer], gp[2 * q.layer + 1], dfrow + q.da_region * kFilmRow, q.cols, q.w_ld,
                                        q.w_col0, q.bias};
            n_chains += q.bias;
            return 0;
        });
        hipLaunchKernelGGL(film_finish_kernel, dim3(256, n_chains), dim3(256), 0, stream, fb);
    }
    return check_launch("film_finish_kernel");
}

// Backward of a field over P points.  grad_params[2i], [2i+1]: device pointers to the weight /
// bias gradient tensors (torch layout), overwritten.
int launch_field_backward(int kind_in, const float* packed_bwd, const float* acts, float* grads, const float* raw,
                          const float* g_raw, int64_t n_groups, int64_t points_per_group, const float* film,
                          float* film_partial, float* grad_film, float* partial, float* const* gp,
                          const float* const* params, hipStream_t stream) {
    const int64_t P = n_groups * points_per_group;
    if (P <= 0) return 0;
    if (bad_kind(kind_in)) return -1;
    const int kind = canon_kind(kind_in);
    const bool film_kind = is_film(kind);
    if (film_kind && (!film || !film_partial || !grad_film || !params)) {
        set_error("FiLM backward needs film, the FiLM scratch, grad_film and the parameter pointers");
        return -1;
    }
    const int64_t tpg = (points_per_group + 127) / 128;
    BwdArgs a{packed_bwd, acts, grads, raw, g_raw, P, film, film_partial, points_per_group, tpg, n_groups * tpg, nullptr, film_depth(kind)};
    const unsigned blocks = (unsigned)(film_kind ? n_groups * tpg : (P + 127) / 128);
    int rc;
    if ((rc = launch_bwd_chain(kind, a, blocks, stream))) return rc;
    const FieldKind& K = field_kind(kind);
    if (!film_kind)
        return plan_then_run(kind, P, P, partial, stream, [&](BwdBatcher& bb) { return batched_backward(K, bb, acts, grads, gp, any_block); });
    if ((rc = film_images_backward(kind, acts, grads, n_groups, points_per_group, film, film_partial, grad_film, partial, gp, params, stream)))
        return rc;
    // heads: no FiLM in between, all images at once
    return plan_then_run(kind, P, P, partial, stream, [&](BwdBatcher& hb) { return batched_backward(K, hb, acts, grads, gp, head_block); });
}

// Backward of a non-FiLM field over the first *count rows of compact acts (the list-driven training forward left them): the
// counted chain, then the pass's weight-gradient jobs planned from the capacity P and run over the device count.  Every grid
// is sized from P; nothing is read back.
int launch_field_backward_list(int kind_in, const float* packed_bwd, const float* acts, float* grads, const float* raw,
                               const float* g_raw, const int* list, const int* count, int64_t P, float* partial,
                               float* const* gp, hipStream_t stream) {
    if (P <= 0) return 0;
    if (bad_kind(kind_in)) return -1;
    const int kind = canon_kind(kind_in);
    CountedBwdArgs a{{packed_bwd, acts, grads, raw, g_raw, P, nullptr, nullptr, P, (P + 127) / 128, (P + 127) / 128, nullptr, 0}, list, count};
    if (const int rc = launch_bwd_chain_counted(kind, a, (unsigned)((P + 127) / 128), stream)) return rc;
    return plan_then_run(kind, P, P, partial, stream,
                         [&](BwdBatcher& bb) { return batched_backward(kFieldKinds[kind], bb, acts, grads, gp, any_block); }, true, count);
}

static int64_t batched_partial_floats(int kind, int64_t P) {
    // Plan only (partial == nullptr: nothing is launched, nothing dereferenced).  The gradient pointers must be NON-null
    // here: a job's record is TM*TK floats plus TM bias sums when it has a bias destination, and a plan made with null
    // destinations comes out 256 floats per record short of what the real pass writes.
    static float sink;
    float* gp[2 * kMaxLayers];
    for (float*& g : gp) g = &sink;
    BwdBatcher bb{P, nullptr, 0, nullptr};
    (void)batched_backward(kFieldKinds[kind], bb, nullptr, nullptr, gp, any_block);
    return bb.used + 1024;
}

}  // namespace mi

