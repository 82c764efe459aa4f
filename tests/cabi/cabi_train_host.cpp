// A torch-free trainer on the C ABI (include/mi_render.h): K steps of nerf/train_nerf.py:151-168 - render_rays, the loss,
// loss.backward(), optimizer.step() - as mi_render_rays_train -> mi_nerf_loss -> mi_render_rays_backward -> mi_adam_step
// on the program's own hipMalloc'd buffers and its own hipStream_t.  TEST INFRASTRUCTURE: tests/test_gpu_cabi_train.py
// runs mirender's own loop (autograd.render_rays_train, train.nerf_loss, train.FusedAdam, train.decayed_lr) from the
// same start and compares the bytes this program writes.  Nothing here computes anything on the device itself.
//
//   cabi_train_host <kind> <shared 0|1> <groups> <width> <height> <n_coarse> <n_fine> <steps> <lr> <lr_decay>
//                   <tables.bin> <out.bin>
//
// tables.bin: z_lin [Nc] then u_lin [Nf] (torch.linspace's tables, fp32).  Weights and the FiLM table come from the
// splitmix64 stream of cabi_host.cpp, the targets (r, g, b, alpha) = 0.5 + U(+-0.5) from seed 4242; the jitter is drawn
// on the device, seed 100 + step, ray0 = 0.  `groups` images (FiLM kinds) share one camera and differ in their FiLM rows.
// Writes, as little-endian fp32: the final parameters (field 0, then field 1 unless shared, state-dict order), the last
// step's loss vector [4], its outputs rgb_c[n,3] depth_c[n] acc_c[n] rgb_f[n,3] depth_f[n] acc_f[n], and for FiLM kinds
// its grad_film [groups,9,512].
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mi_render.h"

#define CHECK_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)
#define CHECK_MI(x) do { int rc_ = (x); if (rc_ != 0) { std::fprintf(stderr, "%s failed (%d): %s\n", #x, rc_, mi_last_error()); return 3; } } while (0)

struct Rng {          // cabi_host.cpp's
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    float uniform(float bound) { return (float)((double)(next() >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0) * bound; }
};

template <class T>
static int upload(T** dst, const std::vector<T>& src, hipStream_t s) {
    CHECK_HIP(hipMalloc(dst, src.size() * sizeof(T) + 16));
    CHECK_HIP(hipMemcpyAsync(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, s));
    CHECK_HIP(hipStreamSynchronize(s));
    return 0;
}

static int zeros(float** dst, size_t count, hipStream_t s) {
    CHECK_HIP(hipMalloc(dst, count * sizeof(float) + 16));
    CHECK_HIP(hipMemsetAsync(*dst, 0, count * sizeof(float), s));
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 13) {
        std::fprintf(stderr, "usage: %s kind shared groups width height n_coarse n_fine steps lr lr_decay tables.bin out.bin\n", argv[0]);
        return 1;
    }
    const int kind = std::atoi(argv[1]), shared = std::atoi(argv[2]) != 0, groups = std::atoi(argv[3]);
    const int W = std::atoi(argv[4]), H = std::atoi(argv[5]), nc = std::atoi(argv[6]), nf = std::atoi(argv[7]);
    const int steps = std::atoi(argv[8]);
    const double lr0 = std::atof(argv[9]), lr_decay = std::atof(argv[10]);
    const bool film_kind = kind == MI_FIELD_FILM_SIREN_NERF || kind == MI_FIELD_FILM_SIREN_NERF_NODIR;
    if (mi_abi_version() != 4) { std::fprintf(stderr, "ABI version %d\n", mi_abi_version()); return 1; }
    if (groups < 1 || (!film_kind && groups != 1)) { std::fprintf(stderr, "groups > 1 needs a FiLM kind\n"); return 1; }
    const int64_t rpg = (int64_t)W * H, n = rpg * groups;
    hipStream_t stream;
    CHECK_HIP(hipStreamCreate(&stream));

    // linspace tables written by the test
    std::vector<float> tables((size_t)nc + nf);
    {
        FILE* f = std::fopen(argv[11], "rb");
        if (!f || std::fread(tables.data(), 4, tables.size(), f) != tables.size()) { std::fprintf(stderr, "cannot read %s\n", argv[11]); return 1; }
        std::fclose(f);
    }
    float *z_lin, *u_lin = nullptr;
    if (upload(&z_lin, std::vector<float>(tables.begin(), tables.begin() + nc), stream)) return 2;
    if (nf > 0 && upload(&u_lin, std::vector<float>(tables.begin() + nc, tables.end()), stream)) return 2;

    // the fields: parameters, Adam moments, gradients, both packed streams
    const int n_fields = shared ? 1 : 2;
    const int n_params = mi_field_num_params(kind);
    if (n_params <= 0) { std::fprintf(stderr, "%s\n", mi_last_error()); return 1; }
    std::vector<float*> params, grads, m1, m2;
    std::vector<int64_t> numel;
    float* packed[2] = {nullptr, nullptr};
    float* packed_bwd[2] = {nullptr, nullptr};
    for (int m = 0; m < n_fields; ++m) {
        Rng rng{1000ull + (uint64_t)m};
        for (int l = 0; l < n_params / 2; ++l) {
            int64_t o, i;
            CHECK_MI(mi_field_param_shape(kind, 2 * l, &o, &i));
            const bool sin_layer = kind != MI_FIELD_NERF && kind != MI_FIELD_TINY_NERF && o != 1 && o != 3;
            const float bound = std::sqrt(6.0f / (float)i) * (sin_layer ? (i <= 3 ? 0.25f : 0.03125f) : 0.875f);
            std::vector<float> w((size_t)o * i), b((size_t)o);
            for (auto& x : w) x = rng.uniform(bound);
            for (auto& x : b) x = rng.uniform(0.05f);
            for (auto* v : {&w, &b}) {
                float *p, *g, *a, *q;
                if (upload(&p, *v, stream) || zeros(&g, v->size(), stream) || zeros(&a, v->size(), stream) ||
                    zeros(&q, v->size(), stream)) return 2;
                params.push_back(p); grads.push_back(g); m1.push_back(a); m2.push_back(q); numel.push_back((int64_t)v->size());
            }
        }
        CHECK_HIP(hipMalloc(&packed[m], (size_t)mi_field_packed_floats(kind) * 4));
        CHECK_HIP(hipMalloc(&packed_bwd[m], (size_t)mi_field_packed_bwd_floats(kind) * 4));
        CHECK_MI(mi_field_pack(kind, params.data() + m * n_params, n_params, 30.0f, packed[m], stream));
        CHECK_MI(mi_field_pack_bwd(kind, params.data() + m * n_params, n_params, 30.0f, packed_bwd[m], stream));
    }
    if (shared) { packed[1] = packed[0]; packed_bwd[1] = packed_bwd[0]; }
    float** p_c = params.data();
    float** p_f = params.data() + (shared ? 0 : n_params);
    float** g_c = grads.data();
    float** g_f = grads.data() + (shared ? 0 : n_params);

    float* film = nullptr;
    float* grad_film = nullptr;
    if (film_kind) {                                     // image g: gamma ~ 1, beta ~ 0, from seed 77 + g
        std::vector<float> f((size_t)groups * 9 * 512);
        for (int g = 0; g < groups; ++g) {
            Rng rng{77ull + (uint64_t)g};
            for (int j = 0; j < 9 * 512; ++j) f[(size_t)g * 9 * 512 + j] = ((j % 512) < 256 ? 1.0f : 0.0f) + rng.uniform(0.25f);
        }
        if (upload(&film, f, stream) || zeros(&grad_film, f.size(), stream)) return 2;
    }

    // rays of one camera (cabi_host.cpp's), repeated for every image; targets
    const float r = film_kind ? 1.0f : 4.0f;
    const float c2w[12] = {0.96f, 0.0f, 0.28f, 0.3f, 0.0f, 1.0f, 0.0f, -0.2f, -0.28f, 0.0f, 0.96f, r};
    const double focal = film_kind ? W / 2.0 / 0.10510423526567646 : 1.3875 * W;
    const float near_ = film_kind ? 0.5f : 2.0f, far_ = film_kind ? 1.5f : 6.0f;
    float* rays;
    CHECK_HIP(hipMalloc(&rays, (size_t)n * 6 * 4));
    CHECK_MI(mi_gen_rays(W, H, focal, c2w, 0, rpg, rays, 0, stream));
    for (int g = 1; g < groups; ++g)
        CHECK_HIP(hipMemcpyAsync(rays + (size_t)g * rpg * 6, rays, (size_t)rpg * 6 * 4, hipMemcpyDeviceToDevice, stream));
    std::vector<float> tgt((size_t)n * 4);
    {
        Rng rng{4242};
        for (auto& x : tgt) x = 0.5f + rng.uniform(0.5f);
    }
    float* target;
    if (upload(&target, tgt, stream)) return 2;

    // buffers of one step.  Range split: autograd._max_points_per_chunk's (48 GiB of saved inputs + per-layer gradients
    // per range, at least 4096 points), so the gradients are summed in the same ranges as mirender's own loop.
    const int64_t per_point = 4 * (mi_field_train_acts_floats(kind) + mi_field_train_grads_floats(kind));
    const int64_t range_points = (48ll << 30) / per_point > 4096 ? (48ll << 30) / per_point : 4096;
    int64_t ws_bytes = mi_render_workspace_bytes(n, nc, nf);
    if (shared) ws_bytes += mi_render_shared_field_extra_bytes(n, nc, nf);
    const int64_t saved_bytes = mi_render_train_saved_bytes(kind, kind, shared, n, nc, nf);
    const int64_t bwd_bytes = mi_render_backward_workspace_bytes(kind, kind, shared, film_kind ? groups : 1,
                                                                 film_kind ? rpg : n, nc, nf, range_points, range_points);
    if (saved_bytes < 0 || bwd_bytes < 0) { std::fprintf(stderr, "%s\n", mi_last_error()); return 1; }
    void *ws, *saved, *bwd_ws;
    float *out, *seeds, *loss_ws, *loss;
    CHECK_HIP(hipMalloc(&ws, (size_t)ws_bytes));
    CHECK_HIP(hipMalloc(&saved, (size_t)saved_bytes));
    CHECK_HIP(hipMalloc(&bwd_ws, (size_t)bwd_bytes));
    CHECK_HIP(hipMalloc(&out, (size_t)n * 10 * 4));
    CHECK_HIP(hipMalloc(&seeds, (size_t)n * 8 * 4));
    CHECK_HIP(hipMalloc(&loss_ws, (size_t)mi_nerf_loss_workspace_floats(n) * 4));
    CHECK_HIP(hipMalloc(&loss, 4 * 4));
    float *rgb_c = out, *depth_c = out + 3 * n, *acc_c = out + 4 * n, *rgb_f = out + 5 * n, *depth_f = out + 8 * n, *acc_f = out + 9 * n;
    float *g_rgb_c = seeds, *g_acc_c = seeds + 3 * n, *g_rgb_f = seeds + 4 * n, *g_acc_f = seeds + 7 * n;
    const int64_t ng = film_kind ? groups : 1, rays_pg = film_kind ? rpg : n;
    const int kinds[2] = {kind, kind};
    const double beta1 = 0.9, beta2 = 0.999, eps = 1e-8;

    for (int step = 0; step < steps; ++step) {
        // train_nerf.py:151-156: render_rays
        CHECK_MI(mi_render_rays_train(kind, packed[0], kind, packed[1], film, rays, ng, rays_pg, near_, far_, nc, nf, z_lin,
                                      u_lin, nullptr, 100 + (uint64_t)step, 0, rgb_c, depth_c, acc_c, rgb_f, depth_f, acc_f,
                                      ws, ws_bytes, range_points, range_points, saved, saved_bytes, stream));
        // :158-166 the loss and the gradient seeds (use_alpha; the coarse loss counts with a separate fine model)
        CHECK_MI(mi_nerf_loss(n, rgb_c, acc_c, rgb_f, acc_f, target, 1, !shared, g_rgb_c, g_acc_c, g_rgb_f, g_acc_f, loss_ws,
                              loss, stream));
        // :167 loss.backward()
        int written = 0;
        CHECK_MI(mi_render_rays_backward(kind, packed[0], packed_bwd[0], p_c, kind, packed[1], packed_bwd[1], p_f, film, rays,
                                         ng, rays_pg, nc, nf, range_points, range_points, ws, ws_bytes, saved, saved_bytes,
                                         g_rgb_c, nullptr, g_acc_c, g_rgb_f, nullptr, g_acc_f, g_c, shared ? nullptr : g_f,
                                         grad_film, bwd_ws, bwd_bytes, &written, stream));
        if (!(written & MI_WROTE_COARSE) || (!shared && !(written & MI_WROTE_FINE))) { std::fprintf(stderr, "fields_written %d\n", written); return 1; }
        // :168 optimizer.step() at train.decayed_lr's rate (:170-175), torch's scalars in double
        const int t = step + 1;
        const double lr = lr0 * std::pow(0.1, step / (lr_decay * 1000));
        const double bc1 = 1 - std::pow(beta1, t), bc2_sqrt = std::sqrt(1 - std::pow(beta2, t));
        CHECK_MI(mi_adam_step(n_fields, kinds, params.data(), grads.data(), m1.data(), m2.data(), numel.data(),
                              (float)(-lr / bc1), (float)(1 - beta1), (float)beta2, (float)(1 - beta2), (float)eps,
                              (float)bc2_sqrt, packed, packed_bwd, stream));
    }

    std::vector<float> host;
    for (size_t i = 0; i < params.size(); ++i) {
        std::vector<float> v((size_t)numel[i]);
        CHECK_HIP(hipMemcpyAsync(v.data(), params[i], v.size() * 4, hipMemcpyDeviceToHost, stream));
        CHECK_HIP(hipStreamSynchronize(stream));
        host.insert(host.end(), v.begin(), v.end());
    }
    const size_t tail = 4 + (size_t)n * 10 + (film_kind ? (size_t)groups * 9 * 512 : 0);
    std::vector<float> rest(tail);
    CHECK_HIP(hipMemcpyAsync(rest.data(), loss, 4 * 4, hipMemcpyDeviceToHost, stream));
    CHECK_HIP(hipMemcpyAsync(rest.data() + 4, out, (size_t)n * 10 * 4, hipMemcpyDeviceToHost, stream));
    if (film_kind)
        CHECK_HIP(hipMemcpyAsync(rest.data() + 4 + n * 10, grad_film, (size_t)groups * 9 * 512 * 4, hipMemcpyDeviceToHost, stream));
    CHECK_HIP(hipStreamSynchronize(stream));
    host.insert(host.end(), rest.begin(), rest.end());
    FILE* f = std::fopen(argv[12], "wb");
    if (!f || std::fwrite(host.data(), 4, host.size(), f) != host.size()) { std::fprintf(stderr, "cannot write %s\n", argv[12]); return 1; }
    std::fclose(f);
    std::printf("cabi_train_host: kind %d shared=%d %d x %dx%d %d+%d, %d steps: loss %.6f\n", kind, shared, groups, W, H, nc,
                nf, steps, (double)rest[0]);
    return 0;
}
