// adam_step.hip - writers of the packed weight streams (field_layout.h) of every field kind (gfx950): the pack kernel,
// and the optimiser step of nerf/train_nerf.py:98,168 (torch.optim.Adam, betas (0.9, 0.999), no weight decay, no amsgrad)
// for the parameters of up to two fields, FUSED with the refresh of their streams.
//
// pack_kernel writes a whole stream, forward or transposed, from the parameter tensors (mi_field_pack /
// mi_field_pack_bwd).  After a torch optimiser step the renderer would have to repack both streams of each model that
// way: two optimiser-side launches and four pack launches per step, on a step that is launch-bound at the reference's
// 1024-ray batch.  adam_pack_kernel does all of it in one launch: thread = one parameter element; it applies Adam to
// (p, m, v) and SCATTERS the new value to every position of the two streams that holds it, by inverting the item tables
// (an element sits in at most a few items: its K block of the forward stream, its K block of the transposed stream, a
// VEC / PLAIN piece for biases, head rows and K = 3 columns).  Padding entries of the streams never change, so they are
// written once by pack_kernel and left alone.
//
// Arithmetic follows torch's multi-tensor Adam op by op (torch/optim/adam.py:_multi_tensor_adam): lerp of exp_avg,
// mul + addcmul of exp_avg_sq, sqrt / bias_correction2_sqrt + eps, addcdiv with -lr / bias_correction1; the scalars
// are computed on the host in double like torch does and handed over as floats.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "field_kinds_host.h"
#include "launchers.h"

namespace mi {

// the only device copies of the item tables: one pair per FIXED kind.  The MI_FIELD_FILM_DEPTH kinds have none (eighteen more
// pairs of 5.6 KB tables do not fit in the 64 KB of constant memory): their tables are regular in the depth, so the kernels
// below compute the item they need from (depth, use_dir, i) with film_item() - the same recipe build_film() runs.
__constant__ PackTable c_fwd[MI_FIELD_KINDS] = {kFieldKinds[0].fwd, kFieldKinds[1].fwd, kFieldKinds[2].fwd, kFieldKinds[3].fwd,
                                                kFieldKinds[4].fwd};
__constant__ PackTable c_bwd[MI_FIELD_KINDS] = {kFieldKinds[0].bwd, kFieldKinds[1].bwd, kFieldKinds[2].bwd, kFieldKinds[3].bwd,
                                                kFieldKinds[4].bwd};

struct PackSrc { const float* p[2 * kMaxLayers]; };

// Item i of a kind's forward (dir = STREAM_FWD) or transposed stream and its float offset; items / body floats of the stream.
__device__ __forceinline__ PickedItem stream_item(int kind, int dir, int i) {
    if (kind < MI_FIELD_KINDS) {
        const PackTable& t = dir == STREAM_FWD ? c_fwd[kind] : c_bwd[kind];
        return {t.item[i], t.dst_off[i]};
    }
    return film_item(depth_of_id(kind), (kind & 1) != 0, dir != STREAM_FWD, i);
}
__device__ __forceinline__ int stream_items(int kind, int dir) {
    if (kind < MI_FIELD_KINDS) return (dir == STREAM_FWD ? c_fwd[kind] : c_bwd[kind]).n_items;
    return film_n_items(depth_of_id(kind), (kind & 1) != 0, dir != STREAM_FWD);
}
__device__ __forceinline__ int stream_body_floats(int kind, int dir) {
    if (kind < MI_FIELD_KINDS) return packed_body_floats(dir == STREAM_FWD ? c_fwd[kind] : c_bwd[kind]);
    return film_body_floats(depth_of_id(kind), (kind & 1) != 0, dir != STREAM_FWD);
}

// grid: (32, n_items); block 256.  One block row per item of the kind's forward (dir = STREAM_FWD) or transposed table.
__global__ void pack_kernel(int kind, int dir, PackSrc src_params, float* __restrict__ dst, float w0) {
    const int it = blockIdx.y;
    if (it >= stream_items(kind, dir)) return;
    if (it == 0 && blockIdx.x == 0) {                        // the trailer piece: hyper-parameters (field_layout.h:kTrailer)
        float* tr = dst + stream_body_floats(kind, dir);
        tr[threadIdx.x] = threadIdx.x == 0 ? w0 : (threadIdx.x == 1 ? w0 * w0 : 0.f);
    }
    const PickedItem picked = stream_item(kind, dir, it);
    const PackItem item = picked.it;
    float* out = dst + picked.off;
    const float* src = src_params.p[item.param];
    if (item.type == ITEM_CHUNK) {
        const int total = item.mb * 1024;
        for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += 32 * 256) {
            int q = idx & 3, lane = (idx >> 2) & 63, rm = idx >> 8;
            int m = rm % item.mb, rg = rm / item.mb;
            int row = 32 * m + (lane & 31);
            int c = 8 * rg + 4 * (lane >> 5) + q;
            float v = 0.f;
            if (row < item.rows_valid && c < item.n_valid)
                v = src[(int64_t)row * item.ld + item.offset + (int64_t)c * item.stride];
            out[idx] = v;
        }
    } else if (blockIdx.x == 0) {
        const int f = threadIdx.x;  // 256 features per piece
        if (item.type == ITEM_VEC) out[vec_slot(f)] = f < item.n_valid ? src[item.offset + (int64_t)f * item.stride] : 0.f;
        else out[f] = f < item.n_valid ? src[f] : 0.f;
    }
}

int launch_pack(int kind_in, StreamDir dir, const float* const* params, int n_params, float w0, float* packed, hipStream_t stream) {
    const int kind = canon_kind(kind_in);
    PackSrc src{};
    for (int i = 0; i < n_params && i < 2 * kMaxLayers; ++i) src.p[i] = params[i];
    const PackTable& t = dir == STREAM_FWD ? field_kind(kind).fwd : field_kind(kind).bwd;
    hipLaunchKernelGGL(pack_kernel, dim3(32, t.n_items), dim3(256), 0, stream, kind, (int)dir, src, packed, w0);
    return check_launch("pack_kernel");
}

constexpr int kAdamMaxParams = 64;      // two fields of up to 30 tensors (FilmSirenNeRF of depth 12)
constexpr int kAdamMaxHits = 16;        // stream items per parameter tensor the kernel's hit lists hold

// The hit lists are sized by a constant, the tables by field_layout.h: tie the two at compile time, so a layout change
// that puts a tensor into more items than the lists hold cannot leave stream positions silently stale.
constexpr int max_items_per_param(const PackTable& t) {
    int worst = 0;
    for (int prm = 0; prm < 2 * kMaxLayers; ++prm) {
        int n = 0;
        for (int i = 0; i < t.n_items; ++i) n += t.item[i].param == prm;
        worst = n > worst ? n : worst;
    }
    return worst;
}
constexpr int max_items_per_param_all() {
    int worst = 0;
    for (const FieldKind& k : kFieldKinds)
        for (const PackTable* t : {&k.fwd, &k.bwd}) { const int n = max_items_per_param(*t); worst = n > worst ? n : worst; }
    for (int L : {kFilmDepthMin, kFilmDepthMax})              // the depth kinds' per-tensor item counts do not depend on L
        for (bool d : {false, true}) {
            const FieldKind k = make_film_kind(L, d);
            for (const PackTable* t : {&k.fwd, &k.bwd}) { const int n = max_items_per_param(*t); worst = n > worst ? n : worst; }
        }
    return worst;
}
static_assert(max_items_per_param_all() <= kAdamMaxHits, "adam_pack_kernel: a parameter sits in more stream items than hit_f / hit_b hold");
struct AdamArgs {
    float* p[kAdamMaxParams];
    const float* g[kAdamMaxParams];
    float* m[kAdamMaxParams];
    float* v[kAdamMaxParams];
    int numel[kAdamMaxParams];
    int in_f[kAdamMaxParams];           // row length of the tensor ([out, in] weight: in; bias: 1)
    int field[kAdamMaxParams];          // which field the tensor belongs to (0 / 1)
    int index[kAdamMaxParams];          // its index in that field's parameter list (the `param` of PackItem)
    int kind[2];
    float* packed_fwd[2];
    float* packed_bwd[2];               // null: the transposed stream does not exist yet (built on first backward)
    float step_size, w1, beta2, w2, eps, bc2_sqrt;   // -lr / bc1, 1 - beta1, beta2, 1 - beta2
};

// Position of the parameter element at (row, col) of its [out, in] matrix (a bias: (f, 0)) in the item's packed image,
// or -1 (see pack_kernel for the forward mapping).  No division: the items carry their first element's coordinates.
__device__ __forceinline__ int packed_index(const PackItem& it, int row, int col) {
    if (it.type == ITEM_PLAIN) return row < it.n_valid ? row : -1;                    // bias scalars at [0..n)
    int r = row - it.row0, c = col - it.col0;
    if (it.type == ITEM_VEC) {
        int f;
        if (it.ld == 0) f = row;                                                      // a bias vector
        else if (it.stride == 1) { if (r != 0) return -1; f = c; }                    // a row of the weight
        else { if (c != 0) return -1; f = r; }                                        // a column of the weight
        return (f >= 0 && f < it.n_valid) ? vec_slot(f) : -1;
    }
    if (it.stride != 1) { const int t = r; r = c; c = t; }                            // transposed K block: MFMA rows = inputs
    if (r < 0 || c < 0 || r >= it.rows_valid || c >= it.n_valid) return -1;
    const int m = r >> 5, lane = (r & 31) + 32 * ((c >> 2) & 1), rg = c >> 3, q = c & 3;
    return (((rg * it.mb + m) * 64 + lane) << 2) + q;
}

// DEPTH = false: both fields are fixed kinds, items are read from the constant tables.  DEPTH = true: a field may be a
// MI_FIELD_FILM_DEPTH kind; the items that hold the block's tensor are computed (or copied) once into LDS.
template <bool DEPTH>
__global__ __launch_bounds__(256) void adam_pack_kernel(AdamArgs a) {
    const int t = blockIdx.y;
    const int n = a.numel[t], in_f = a.in_f[t];
    const int fld = a.field[t], prm = a.index[t];
    const int kind = a.kind[fld];
    const PackTable& tf = c_fwd[DEPTH ? 0 : kind];
    const PackTable& tb = c_bwd[DEPTH ? 0 : kind];
    float* pf = a.packed_fwd[fld];
    float* pb = a.packed_bwd[fld];
    // the items that hold this tensor, found once per block (a tensor sits in <= 10 forward and <= 9 transposed items;
    // walking both 100-item tables per ELEMENT cost 130 us on a 1.2 M-parameter step)
    // (thread i looks at item i of each table; the order of the hits does not matter, every hit writes its own positions)
    if (blockIdx.x * 256 >= n) return;                           // the grid is sized for the largest tensor
    __shared__ int hit_f[kAdamMaxHits], hit_b[kAdamMaxHits], n_hit[2];
    __shared__ PickedItem sh_f[DEPTH ? kAdamMaxHits : 1], sh_b[DEPTH ? kAdamMaxHits : 1];
    if (threadIdx.x < 2) n_hit[threadIdx.x] = 0;
    __syncthreads();
    if constexpr (DEPTH) {
        for (int i = threadIdx.x, ni = stream_items(kind, STREAM_FWD); i < ni; i += 256) {
            const PickedItem q = stream_item(kind, STREAM_FWD, i);
            if (q.it.param == prm) { const int k = atomicAdd(&n_hit[0], 1); if (k < kAdamMaxHits) sh_f[k] = q; }
        }
        if (pb)
            for (int i = threadIdx.x, ni = stream_items(kind, STREAM_BWD); i < ni; i += 256) {
                const PickedItem q = stream_item(kind, STREAM_BWD, i);
                if (q.it.param == prm) { const int k = atomicAdd(&n_hit[1], 1); if (k < kAdamMaxHits) sh_b[k] = q; }
            }
    } else {
        for (int i = threadIdx.x; i < tf.n_items; i += 256)
            if (tf.item[i].param == prm) { const int k = atomicAdd(&n_hit[0], 1); if (k < kAdamMaxHits) hit_f[k] = i; }
        if (pb)
            for (int i = threadIdx.x; i < tb.n_items; i += 256)
                if (tb.item[i].param == prm) { const int k = atomicAdd(&n_hit[1], 1); if (k < kAdamMaxHits) hit_b[k] = i; }
    }
    __syncthreads();
    const int nf = n_hit[0], nb = n_hit[1];                      // <= kAdamMaxHits by the static_assert above
    for (int e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
        const float g = a.g[t][e];
        float m = a.m[t][e], v = a.v[t][e], p = a.p[t][e];
        m = m + a.w1 * (g - m);                                  // exp_avg.lerp_(grad, 1 - beta1)
        v = v * a.beta2;                                         // exp_avg_sq.mul_(beta2)
        v = v + (a.w2 * g) * g;                                  //            .addcmul_(grad, grad, value = 1 - beta2)
        const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
        p = p + a.step_size * (m / denom);                       // param.addcdiv_(exp_avg, denom, value = -lr / bc1)
        a.m[t][e] = m; a.v[t][e] = v; a.p[t][e] = p;
        const int row = e / in_f, col = e - row * in_f;
        if constexpr (DEPTH) {
            for (int h = 0; h < nf; ++h) {
                const int k = packed_index(sh_f[h].it, row, col);
                if (k >= 0) pf[sh_f[h].off + k] = p;
            }
            for (int h = 0; h < nb; ++h) {
                const int k = packed_index(sh_b[h].it, row, col);
                if (k >= 0) pb[sh_b[h].off + k] = p;
            }
        } else {
            for (int h = 0; h < nf; ++h) {
                const int i = hit_f[h], k = packed_index(tf.item[i], row, col);
                if (k >= 0) pf[tf.dst_off[i] + k] = p;
            }
            for (int h = 0; h < nb; ++h) {
                const int i = hit_b[h], k = packed_index(tb.item[i], row, col);
                if (k >= 0) pb[tb.dst_off[i] + k] = p;
            }
        }
    }
}

int launch_adam_step(int n_fields, const int* kinds, const int* n_params, float* const* params, const float* const* grads,
                     float* const* exp_avg, float* const* exp_avg_sq, const int64_t* numel, float step_size,
                     float one_minus_beta1, float beta2, float one_minus_beta2, float eps, float bc2_sqrt,
                     float* const* packed_fwd, float* const* packed_bwd, hipStream_t stream) {
    AdamArgs a{};
    int t = 0;
    int64_t most = 0;
    bool depth = false;
    for (int f = 0; f < n_fields; ++f) {
        a.kind[f] = canon_kind(kinds[f]);
        depth |= is_depth_kind(a.kind[f]);
        a.packed_fwd[f] = packed_fwd[f];
        a.packed_bwd[f] = packed_bwd ? packed_bwd[f] : nullptr;
        for (int i = 0; i < n_params[f]; ++i, ++t) {
            if (t >= kAdamMaxParams) { set_error("mi_adam_step: more than %d tensors", kAdamMaxParams); return -1; }
            if (numel[t] > 0x7fffffff) { set_error("mi_adam_step: tensor too large"); return -1; }
            a.p[t] = params[t]; a.g[t] = grads[t]; a.m[t] = exp_avg[t]; a.v[t] = exp_avg_sq[t];
            a.numel[t] = (int)numel[t]; a.field[t] = f; a.index[t] = i;
            if (!(i & 1) && (numel[t + 1] <= 0 || numel[t] % numel[t + 1] != 0)) {
                set_error("mi_adam_step: tensor %d (%lld elements) is not a [out, in] weight of the bias that follows it (%lld)",
                          t, (long long)numel[t], (long long)numel[t + 1]);
                return -1;
            }
            a.in_f[t] = (i & 1) ? 1 : (int)(numel[t] / numel[t + 1]);          // weight [out, in] is followed by its bias [out]
            if (numel[t] > most) most = numel[t];
        }
    }
    a.step_size = step_size; a.w1 = one_minus_beta1; a.beta2 = beta2; a.w2 = one_minus_beta2; a.eps = eps; a.bc2_sqrt = bc2_sqrt;
    if (t == 0) return 0;
    const unsigned bx = (unsigned)((most + 255) / 256 < 64 ? (most + 255) / 256 : 64);
    if (depth) hipLaunchKernelGGL(adam_pack_kernel<true>, dim3(bx ? bx : 1, t), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(adam_pack_kernel<false>, dim3(bx ? bx : 1, t), dim3(256), 0, stream, a);
    return check_launch("adam_pack_kernel");
}

}  // namespace mi
