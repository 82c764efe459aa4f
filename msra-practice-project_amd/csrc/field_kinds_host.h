// field_kinds_host.h - the host side of the field-kind registry (field_kinds.h): the C ABI's kind check, the descriptor lookup
// and the one walker of a kind's layer graph (for_each_block), from which the weight-gradient jobs of field_bwd_dw.hip and the
// input gradients of ray_grad.hip are derived.  No kernel unit of the MFMA families includes it.
#pragma once
#include <stdint.h>

#include "field_kinds.h"
#include "mi_host.h"

namespace mi {

// Validates a kind from the C ABI; sets the error message if it names none.
inline bool bad_kind(int kind) {
    if (is_depth_id(kind) && !is_depth_kind(kind)) {
        set_error("FiLM depth kind 0x%x: hidden_layers = %d is outside the supported range %d..%d", kind, depth_of_id(kind),
                  kFilmDepthMin, kFilmDepthMax);
        return true;
    }
    if (!is_fixed_kind(kind) && !is_depth_kind(kind)) { set_error("unknown field kind %d", kind); return true; }
    return false;
}

// Descriptor of a VALID kind, fixed or depth (api.hip builds the depth kinds' once, on first use).
const FieldKind& field_kind(int kind);


// ---- the graph's walker (host) -----------------------------------------------------------------------------------------
// One (layer, input) block of a kind's graph over P points, as pointers and strides: dW[rows][w_ld] at column w_col0 is
// sum_p dA[p][da_c0 + r] X[p][x_c0 + c].  The bias gradient rides with the layer's hidden input, or with its only input.
struct GraphBlock {
    int layer;                                 // parameter pair: weight 2 * layer, bias 2 * layer + 1
    int cls;                                   // SrcClass of the input
    bool head, bias;
    int da_region;                             // FiLM kinds, non-head layers: the layer's FiLM row
    const float* dA; int da_ld, da_c0, rows;   // [points][da_ld] rows of grads; valid rows of dW
    const float* X; int x_ld, x_c0, cols;      // [points][x_ld] rows of acts; valid columns of the block
    int w_ld, w_col0;
};
// Visits every block in layer order, inputs in weight-column order.  Rows start at point p0 of the P the buffers hold (a
// FiLM image's first point).  Null buffers give null-based pointers for plan-only runs: never dereferenced.
template <class F>
void for_each_block(const FieldKind& K, const float* acts, const float* grads, int64_t P, int64_t p0, F&& f) {
    for (int i = 0; i < K.n_layers; ++i) {
        const LayerGraph& g = K.graph[i];
        for (int j = 0, wcol = 0; j < g.n_in; wcol += g.in[j++].width()) {
            const LayerInput& in = g.in[j];
            const int da_ld = K.grads.width[g.da_region], x_ld = K.acts.width[in.region];
            f(GraphBlock{i, in.cls, g.head, in.cls == SRC_HIDDEN || g.n_in == 1, g.da_region,
                         grads + (int64_t)region_offset(K.grads, g.da_region) * P + p0 * da_ld, da_ld, g.da_c0, g.da_c1 - g.da_c0,
                         acts + (int64_t)region_offset(K.acts, in.region) * P + p0 * x_ld, x_ld, in.c0, in.width(),
                         K.dims[i][1], wcol});
        }
    }
}

}  // namespace mi
