// field_kinds.h - the field-kind registry: one compile-time descriptor per MI_FIELD_* kind (include/mi_render.h),
// indexed by the kind's value.  Everything the host code and the pack / Adam kernels need to know about a kind
// (its parameter shapes, its packed weight streams, its training buffers) is read from here.
#pragma once
#include <stdint.h>

#include "../../include/mi_render.h"
#include "field_layout.h"
#include "mi_common.h"

namespace mi {

constexpr int kMaxLayers = 15;           // FilmSirenNeRF with hidden_layers = 12 has 15

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

// FilmSirenNeRF(hidden_dim = 256, hidden_layers = L, use_dir) (pi_GAN/modules.py:73-94): L + 3 linear layers
constexpr FieldKind make_film_kind(int L, bool use_dir) {
    FieldKind k{};
    k.n_layers = L + 3;
    k.dims[0][0] = 256; k.dims[0][1] = 3;
    for (int l = 1; l < L; ++l) { k.dims[l][0] = 256; k.dims[l][1] = 256; }
    k.dims[L][0] = 1; k.dims[L][1] = 256;
    k.dims[L + 1][0] = 256; k.dims[L + 1][1] = use_dir ? 259 : 256;
    k.dims[L + 2][0] = 3; k.dims[L + 2][1] = 256;
    k.film = true; k.use_dir = use_dir;
    k.acts = film_acts_depth(L); k.grads = film_grads_depth(L);
    k.fwd = build_film(use_dir, L); k.bwd = build_film_bwd(use_dir, L);
    k.trunk = L; k.sigma_head = L;
    return k;
}

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
// the depth kinds are not table rows (see field_kind() below); their two ends are checked here all the same
static_assert(region_total(film_acts_depth(8)) == region_total(film_acts()) && region_total(film_grads_depth(8)) == region_total(film_grads()) &&
              film_grads_depth(8).n == film_grads().n, "depth 8 is the literal layout");
static_assert(make_film_kind(8, true).macs() == 526848 && make_film_kind(8, false).macs() == 526080, "depth 8 is kinds 2 / 3");
static_assert(make_film_kind(4, true).macs() == 264704 && make_film_kind(4, false).macs() == 263936, "FilmSirenNeRF depth 4 MACs per point");
static_assert(make_film_kind(12, true).macs() == 788992 && make_film_kind(12, false).macs() == 788224, "FilmSirenNeRF depth 12 MACs per point");
static_assert(make_film_kind(4, true).sigma_prefix_ok() && make_film_kind(4, false).sigma_prefix_ok() &&
                  make_film_kind(12, true).sigma_prefix_ok() && make_film_kind(12, false).sigma_prefix_ok(),
              "every FiLM depth's stream puts the sigma path's weights first");
constexpr bool film_closed_forms_ok(int L, bool use_dir) {
    const FieldKind k = make_film_kind(L, use_dir);
    if (k.fwd.n_items != film_n_items(L, use_dir, false) || k.bwd.n_items != film_n_items(L, use_dir, true)) return false;
    if (packed_body_floats(k.fwd) != film_body_floats(L, use_dir, false)) return false;
    if (packed_body_floats(k.bwd) != film_body_floats(L, use_dir, true)) return false;
    for (int i = 0; i < k.fwd.n_items; i += 7) {
        const PickedItem p = film_item(L, use_dir, false, i);
        if (p.off != k.fwd.dst_off[i] || p.it.param != k.fwd.item[i].param || p.it.type != k.fwd.item[i].type) return false;
    }
    const PickedItem q = film_item(L, use_dir, true, k.bwd.n_items - 1);
    return q.off == k.bwd.dst_off[k.bwd.n_items - 1] && q.it.param == 2 && k.fwd.n_items <= kMaxItems;
}
static_assert(film_closed_forms_ok(4, true) && film_closed_forms_ok(4, false) && film_closed_forms_ok(8, true) &&
                  film_closed_forms_ok(8, false) && film_closed_forms_ok(12, true) && film_closed_forms_ok(12, false),
              "film_n_items / film_body_floats / film_item restate the tables build_film builds");
static_assert(kFieldKinds[MI_FIELD_NERF].sigma_macs() == 489728, "NeRF sigma-path MACs per point");
static_assert(kFieldKinds[MI_FIELD_SIREN_NERF].sigma_macs() == 460544, "SirenNeRF sigma-path MACs per point");
static_assert(kFieldKinds[MI_FIELD_TINY_NERF].sigma_macs() == 212224, "TinyNeRF sigma-path MACs per point");
static_assert(kFieldKinds[MI_FIELD_NERF].sigma_prefix_ok() && kFieldKinds[MI_FIELD_SIREN_NERF].sigma_prefix_ok() &&
                  kFieldKinds[MI_FIELD_FILM_SIREN_NERF].sigma_prefix_ok() &&
                  kFieldKinds[MI_FIELD_FILM_SIREN_NERF_NODIR].sigma_prefix_ok() && kFieldKinds[MI_FIELD_TINY_NERF].sigma_prefix_ok(),
              "every kind's stream puts the sigma path's weights first");

// ---- MI_FIELD_FILM_DEPTH kinds -------------------------------------------------------------------------------------
// A depth kind is no row of kFieldKinds and has no table in constant memory (adam_step.hip keeps one PackTable pair per
// fixed kind there, about 11 KB each; eighteen more do not fit in 64 KB).  The host reads a depth kind's descriptor from
// field_kind(); the kernels take the depth as a run-time argument and compute stream items with film_item().
constexpr bool is_depth_id(int kind) { return kind >= 0x100 && kind < 0x200; }
constexpr int depth_of_id(int kind) { return (kind - 0x100) >> 1; }
constexpr bool is_depth_kind(int kind) {
    return is_depth_id(kind) && depth_of_id(kind) >= kFilmDepthMin && depth_of_id(kind) <= kFilmDepthMax;
}
static_assert(kFilmDepthMin == MI_FIELD_FILM_DEPTH_MIN && kFilmDepthMax == MI_FIELD_FILM_DEPTH_MAX, "header and layout agree");
// Depth 8 IS kinds 2 / 3: normalised wherever a kind selects a kernel or a table, so it gives their bits.
constexpr int canon_kind(int kind) {
    return is_depth_kind(kind) && depth_of_id(kind) == 8 ? ((kind & 1) ? MI_FIELD_FILM_SIREN_NERF : MI_FIELD_FILM_SIREN_NERF_NODIR) : kind;
}
constexpr bool is_fixed_kind(int kind) { return kind >= 0 && kind < MI_FIELD_KINDS; }
constexpr bool is_film(int kind) { return is_depth_kind(kind) || (is_fixed_kind(kind) && kFieldKinds[kind].film); }
// hidden_layers of a FiLM kind (8 for kinds 2 / 3), 0 for the others
constexpr int film_depth(int kind) { return is_depth_kind(kind) ? depth_of_id(kind) : is_film(kind) ? 8 : 0; }
constexpr bool film_use_dir(int kind) { return is_depth_kind(kind) ? (kind & 1) != 0 : kind == MI_FIELD_FILM_SIREN_NERF; }
constexpr int film_layers(int kind) { return is_film(kind) ? film_depth(kind) + 1 : 0; }
constexpr int64_t film_floats(int kind) { return (int64_t)film_layers(kind) * kFilmRow; }   // one group's rows of the FiLM table

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

}  // namespace mi
