// field_kinds.h - the field-kind registry: one compile-time descriptor per MI_FIELD_* kind (include/mi_render.h),
// indexed by the kind's value.  Everything the host code and the pack / Adam kernels need to know about a kind
// (its parameter shapes, its packed weight streams, its training buffers) is read from here.
#pragma once
#include <stdint.h>

#include "../../include/mi_render.h"
#include "field_layout.h"
#include "mi_common.h"

namespace mi {

constexpr int kMaxLayers = 12;

struct FieldKind {
    int n_layers;                  // linear layers: parameters 2i / 2i+1 are the weight / bias of layer i
    int dims[kMaxLayers][2];       // (out, in) of every linear layer in that order (oracle/fields.py SPECS)
    bool film;                     // FilmSirenNeRF: FiLM table per group, per-image backward
    bool use_dir;                  // the rgb branch reads the view direction
    RegionLayout acts, grads;      // training buffers (field_layout.h)
    PackTable fwd, bwd;            // packed weight streams: forward order, and transposed for the backward chain
    int trunk;                     // layers 0 .. trunk-1 are the density trunk: sigma reads the last one's activation
    int sigma_head;                // the sigma head's layer; every other layer is the colour branch

    // multiply-accumulates of the linear layers per point (a6, a7, a8)
    constexpr int64_t macs() const {
        int64_t s = 0;
        for (int l = 0; l < n_layers; ++l) s += (int64_t)dims[l][0] * dims[l][1];
        return s;
    }
    constexpr bool in_sigma_path(int layer) const { return layer < trunk || layer == sigma_head; }
    // ... of the layers sigma depends on (what a sigma-only forward executes)
    constexpr int64_t sigma_macs() const {
        int64_t s = 0;
        for (int l = 0; l < n_layers; ++l)
            if (in_sigma_path(l)) s += (int64_t)dims[l][0] * dims[l][1];
        return s;
    }
    // The sigma prefix of the forward stream: items [0, sigma_items()) hold every weight sigma needs, item sigma_items()
    // starts the colour branch.  A sigma-only forward consumes exactly this prefix of the same packed buffer.
    constexpr int sigma_items() const {
        int i = 0;
        while (i < fwd.n_items && in_sigma_path(fwd.item[i].param / 2)) ++i;
        return i;
    }
    // true if no item of the colour branch sits inside the prefix and no sigma item behind it
    constexpr bool sigma_prefix_ok() const {
        for (int i = 0; i < fwd.n_items; ++i)
            if (in_sigma_path(fwd.item[i].param / 2) != (i < sigma_items())) return false;
        return sigma_items() < fwd.n_items;
    }
    // The first stage of the colour branch, which the last trunk layer issues while its last K blocks compute: its aux
    // (VEC / PLAIN) pieces, and the DMA pieces of one of its K blocks.  A sigma-only forward issues neither.
    constexpr int branch_aux_pieces() const {
        int n = 0;
        for (int i = sigma_items(); i < fwd.n_items && fwd.item[i].type != ITEM_CHUNK; ++i) ++n;
        return n;
    }
    constexpr int branch_block_pieces() const {
        const PackItem& k = fwd.item[sigma_items() + branch_aux_pieces()];
        return k.type == ITEM_CHUNK ? k.mb * 1024 / kPiece : 0;
    }
};

// nerf/nerf.py:59-73, 128-146; pi_GAN/modules.py:76-94; TinyNeRF is build-defined (BASELINE C1)
inline constexpr FieldKind kFieldKinds[MI_FIELD_KINDS] = {
    // MI_FIELD_NERF
    {12, {{256, 60}, {256, 256}, {256, 256}, {256, 256}, {256, 256}, {256, 316}, {256, 256}, {256, 256}, {256, 256},
          {128, 280}, {1, 256}, {3, 128}},
     false, true, nerf_acts(), nerf_grads(), build_nerf(), build_nerf_bwd(), 8, 10},
    // MI_FIELD_SIREN_NERF
    {12, {{256, 3}, {256, 256}, {256, 256}, {256, 256}, {256, 256}, {256, 259}, {256, 256}, {256, 256}, {256, 256},
          {128, 259}, {1, 256}, {3, 128}},
     false, true, siren_acts(), siren_grads(), build_siren_nerf(), build_siren_nerf_bwd(), 8, 10},
    // MI_FIELD_FILM_SIREN_NERF
    {11, {{256, 3}, {256, 256}, {256, 256}, {256, 256}, {256, 256}, {256, 256}, {256, 256}, {256, 256}, {1, 256},
          {256, 259}, {3, 256}},
     true, true, film_acts(), film_grads(), build_film(true), build_film_bwd(true), 8, 8},
    // MI_FIELD_FILM_SIREN_NERF_NODIR
    {11, {{256, 3}, {256, 256}, {256, 256}, {256, 256}, {256, 256}, {256, 256}, {256, 256}, {256, 256}, {1, 256},
          {256, 256}, {3, 256}},
     true, false, film_acts(), film_grads(), build_film(false), build_film_bwd(false), 8, 8},
    // MI_FIELD_TINY_NERF
    {7, {{256, 60}, {256, 256}, {256, 256}, {256, 256}, {128, 280}, {1, 256}, {3, 128}},
     false, true, tiny_acts(), tiny_grads(), build_tiny_nerf(), build_tiny_nerf_bwd(), 4, 5},
};

static_assert(kFieldKinds[MI_FIELD_NERF].macs() == 591488, "NeRF MACs per point");
static_assert(kFieldKinds[MI_FIELD_SIREN_NERF].macs() == 559616, "SirenNeRF MACs per point");
static_assert(kFieldKinds[MI_FIELD_FILM_SIREN_NERF].macs() == 526848, "FilmSirenNeRF MACs per point");
static_assert(kFieldKinds[MI_FIELD_FILM_SIREN_NERF_NODIR].macs() == 526080, "FilmSirenNeRF (no dir) MACs per point");
static_assert(kFieldKinds[MI_FIELD_TINY_NERF].macs() == 248448, "TinyNeRF MACs per point");
static_assert(kFieldKinds[MI_FIELD_NERF].sigma_macs() == 489728, "NeRF sigma-path MACs per point");
static_assert(kFieldKinds[MI_FIELD_SIREN_NERF].sigma_macs() == 460544, "SirenNeRF sigma-path MACs per point");
static_assert(kFieldKinds[MI_FIELD_TINY_NERF].sigma_macs() == 212224, "TinyNeRF sigma-path MACs per point");
static_assert(kFieldKinds[MI_FIELD_NERF].sigma_prefix_ok() && kFieldKinds[MI_FIELD_SIREN_NERF].sigma_prefix_ok() &&
                  kFieldKinds[MI_FIELD_FILM_SIREN_NERF].sigma_prefix_ok() &&
                  kFieldKinds[MI_FIELD_FILM_SIREN_NERF_NODIR].sigma_prefix_ok() && kFieldKinds[MI_FIELD_TINY_NERF].sigma_prefix_ok(),
              "every kind's stream puts the sigma path's weights first");

constexpr bool is_film(int kind) { return kind >= 0 && kind < MI_FIELD_KINDS && kFieldKinds[kind].film; }

// Validates a kind from the C ABI; sets the error message if it names none.
inline bool bad_kind(int kind) {
    if (kind < 0 || kind >= MI_FIELD_KINDS) { set_error("unknown field kind %d", kind); return true; }
    return false;
}

}  // namespace mi
