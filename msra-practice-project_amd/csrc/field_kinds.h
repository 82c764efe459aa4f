// field_kinds.h - the field-kind registry: one compile-time descriptor per MI_FIELD_* kind (include/mi_render_kinds.h),
// indexed by the kind's value.  Everything the host code and the pack / Adam kernels need to know about a kind
// (its parameter shapes, its packed weight streams, its training buffers, and its layer GRAPH: which saved input and which
// weight columns every linear layer multiplies, and where its dA rows live) is read from here.  The graph is stated once,
// by two builders (with_nerf_graph, make_film_kind), checked at compile time (graph_ok) and read by one host-side walker
// (for_each_block, field_kinds_host.h): the weight-gradient jobs of field_bwd_dw.hip and the input gradients of ray_grad.hip
// are derived from it.  The packed streams are held against the graph segment by segment (segments_ok), and the fused MLP kernels read
// their stage shapes from the same segments (field_layout.h).  Host only but for those compile-time reads: the kernels get
// pointers and strides, and constant memory holds the PackTables alone.
#pragma once
#include <stdint.h>

#include "../../include/mi_render_kinds.h"
#include "field_layout.h"

namespace mi {

constexpr int kMaxLayers = 15;           // FilmSirenNeRF with hidden_layers = 12 has 15

// One input of a linear layer: columns [c0, c1) of an acts region.  The class tells a hidden activation from the raw input.
enum SrcClass : int {
    SRC_HIDDEN = 0,            // a whole 256- / 128-wide activation region
    SRC_XIN,                   // the 8-wide xin row: xyz = columns [0, 3), view direction = [3, 6)
    SRC_E_POS,                 // positional encoding of xyz: 60 of 64 columns
    SRC_E_DIR,                 // positional encoding of the direction: 24 of 32 columns
};
struct LayerInput {
    int cls, region, c0, c1;
    constexpr int width() const { return c1 - c0; }
    constexpr bool is_pos() const { return cls == SRC_E_POS || (cls == SRC_XIN && c0 == 0); }
    constexpr bool is_dir() const { return cls == SRC_E_DIR || (cls == SRC_XIN && c0 == 3); }
};
// Linear layer i: its one or two concatenated inputs in the order of the weight's columns (an input's weight column offset
// is the sum of the widths before it), and its dA rows: columns [da_c0, da_c1) of a grads region - the whole region, or for
// the two heads a column range of the four-wide heads region (rgb 0..2, sigma 3).  In a FiLM kind grads region r holds
// dL/du of FiLM row r, so da_region is also the layer's row of an image's FiLM table.
struct LayerGraph {
    int n_in;
    LayerInput in[2];
    int da_region, da_c0, da_c1;
    bool head;
};

struct FieldKind {
    int n_layers;                  // linear layers: parameters 2i / 2i+1 are the weight / bias of layer i
    int dims[kMaxLayers][2];       // (out, in) of every linear layer in that order (oracle/fields.py SPECS)
    bool film;                     // FilmSirenNeRF: FiLM table per group, per-image backward
    bool use_dir;                  // the rgb branch reads the view direction
    RegionLayout acts, grads;      // training buffers (field_layout.h)
    PackTable fwd, bwd;            // packed weight streams: forward order, and transposed for the backward chain
    int trunk;                     // layers 0 .. trunk-1 are the density trunk: sigma reads the last one's activation
    int sigma_head;                // the sigma head's layer; every other layer is the colour branch
    LayerGraph graph[kMaxLayers];  // see LayerGraph; filled by with_nerf_graph / make_film_kind

    constexpr LayerInput hidden_in(int region) const { return {SRC_HIDDEN, region, 0, acts.width[region]}; }
    constexpr void layer(int i, int da_region, LayerInput a, LayerInput b = {}) {
        graph[i] = {b.c1 > b.c0 ? 2 : 1, {a, b}, da_region, 0, grads.width[da_region], false};
    }
    constexpr void head(int i, int c0, int c1, LayerInput a) { graph[i] = {1, {a, {}}, grads.n - 1, c0, c1, true}; }

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
    constexpr int rgb_head() const { return n_layers - 1; }      // the rgb head's layer: every kind's last
    // The sigma prefix of the forward stream, in segments (field_layout.h): segments [0, sigma_segments()) are the trunk's
    // and hold every weight sigma needs - a sigma-only forward consumes exactly this prefix of the same packed buffer.
    // Segment sigma_segments() is the colour branch's first: the last trunk layer issues its aux pieces and first K blocks
    // while its own last K blocks compute (a sigma-only forward issues neither), and a kernel that runs the colour
    // branch alone enters the stream at its float offset.
    constexpr int sigma_segments() const {
        const Segments S = segments(fwd);
        int i = 0;
        while (i < S.n && S.seg[i].layer < trunk) ++i;
        return i;
    }
    // true if no piece of the colour branch sits inside the prefix and no sigma piece behind it
    constexpr bool sigma_prefix_ok() const {
        const Segments S = segments(fwd);
        const int n = sigma_segments();
        for (int i = 0; i < S.n; ++i) {
            const Segment& s = S.seg[i];
            if (in_sigma_path(s.layer) != (i < n)) return false;
            for (int j = 0; j < s.aux && j < kMaxAuxPieces; ++j)
                if (in_sigma_path(s.item[j].layer) != (i < n)) return false;
        }
        return n < S.n;
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
    // acts: 0 xin | 1 + l = X_l;  grads: l = dL/du_l | L + 1 heads.  FiLM row l < L is layer l, row L is hidden_layer_rgb
    k.layer(0, 0, {SRC_XIN, 0, 0, 3});
    for (int l = 1; l < L; ++l) k.layer(l, l, k.hidden_in(l));
    k.head(L, 3, 4, k.hidden_in(L));
    k.layer(L + 1, L, k.hidden_in(L), use_dir ? LayerInput{SRC_XIN, 0, 3, 6} : LayerInput{});
    k.head(L + 2, 0, 3, k.hidden_in(L + 1));
    return k;
}

// NeRF, TinyNeRF, SirenNeRF share one topology: k.trunk position layers (layer l reads acts region l and writes grads region
// l; the skip layer reads [input | h], nerf/nerf.py:84,160), an optional linear layers_dir.0, the dir layer d = [h | direction]
// and the two heads (sigma on the trunk's output, rgb on the dir layer's).  sin: the input is the raw xin row (acts region 0)
// and the dir layer's output is region d + 1; else the encodings E_pos (region 0) and E_dir (region d + 1), output d + 2.
constexpr int kSkipLayer = 5;
constexpr FieldKind with_nerf_graph(FieldKind k, bool sin) {
    const int d = k.n_layers - 3;
    const LayerInput pos = sin ? LayerInput{SRC_XIN, 0, 0, 3} : LayerInput{SRC_E_POS, 0, 0, 60};
    const LayerInput dir = sin ? LayerInput{SRC_XIN, 0, 3, 6} : LayerInput{SRC_E_DIR, d + 1, 0, 24};
    k.layer(0, 0, pos);
    for (int l = 1; l < d; ++l) {
        if (l == kSkipLayer && l < k.trunk) k.layer(l, l, pos, k.hidden_in(l));
        else k.layer(l, l, k.hidden_in(l));
    }
    k.layer(d, d, k.hidden_in(d), dir);
    k.head(d + 1, 3, 4, k.hidden_in(k.trunk));
    k.head(d + 2, 0, 3, k.hidden_in(d + (sin ? 1 : 2)));
    return k;
}

// nerf/nerf.py:59-73, 128-146; pi_GAN/modules.py:76-94; TinyNeRF is build-defined (BASELINE C1)
inline constexpr FieldKind kFieldKinds[MI_FIELD_KINDS] = {
    // MI_FIELD_NERF
    with_nerf_graph({12, {{256, 60}, {256, 256}, {256, 256}, {256, 256}, {256, 256}, {256, 316}, {256, 256}, {256, 256}, {256, 256},
                          {128, 280}, {1, 256}, {3, 128}},
                     false, true, nerf_acts(), nerf_grads(), build_nerf(), build_nerf_bwd(), 8, 10, {}}, false),
    // MI_FIELD_SIREN_NERF
    with_nerf_graph({12, {{256, 3}, {256, 256}, {256, 256}, {256, 256}, {256, 256}, {256, 259}, {256, 256}, {256, 256}, {256, 256},
                          {128, 259}, {1, 256}, {3, 128}},
                     false, true, siren_acts(), siren_grads(), build_siren_nerf(), build_siren_nerf_bwd(), 8, 10, {}}, true),
    make_film_kind(8, true),       // MI_FIELD_FILM_SIREN_NERF: the reference's default depth
    make_film_kind(8, false),      // MI_FIELD_FILM_SIREN_NERF_NODIR
    // MI_FIELD_TINY_NERF
    with_nerf_graph({7, {{256, 60}, {256, 256}, {256, 256}, {256, 256}, {128, 280}, {1, 256}, {3, 128}},
                     false, true, tiny_acts(), tiny_grads(), build_tiny_nerf(), build_tiny_nerf_bwd(), 4, 5, {}}, false),
};

static_assert(kFieldKinds[MI_FIELD_NERF].macs() == 591488, "NeRF MACs per point");
static_assert(kFieldKinds[MI_FIELD_SIREN_NERF].macs() == 559616, "SirenNeRF MACs per point");
static_assert(kFieldKinds[MI_FIELD_FILM_SIREN_NERF].macs() == 526848, "FilmSirenNeRF MACs per point");
static_assert(kFieldKinds[MI_FIELD_FILM_SIREN_NERF_NODIR].macs() == 526080, "FilmSirenNeRF (no dir) MACs per point");
static_assert(kFieldKinds[MI_FIELD_TINY_NERF].macs() == 248448, "TinyNeRF MACs per point");
// the depth kinds are not table rows (see field_kind(), field_kinds_host.h); their two ends are checked here all the same
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

// ---- the graph's compile-time checks ---------------------------------------------------------------------------------
// Every layer's inputs tile its weight's columns exactly, every input is a legal range of a region of its class's width,
// the dA rows are as wide as the layer has outputs, and the kind has no more input-consuming layers than ray_grad.hip's
// InputGradArgs has slots for (two position consumers, one direction consumer).
constexpr bool input_ok(const RegionLayout& A, const LayerInput& in) {
    if (in.region < 0 || in.region >= A.n) return false;
    const int w = A.width[in.region];
    switch (in.cls) {
        case SRC_HIDDEN: return in.c0 == 0 && in.c1 == w && (w == 256 || w == 128);
        case SRC_XIN: return w == 8 && in.c1 == in.c0 + 3 && (in.c0 == 0 || in.c0 == 3);
        case SRC_E_POS: return w == 64 && in.c0 == 0 && in.c1 == 60;
        case SRC_E_DIR: return w == 32 && in.c0 == 0 && in.c1 == 24;
    }
    return false;
}
constexpr bool graph_ok(const FieldKind& k) {
    int n_pos = 0, n_dir = 0;
    for (int i = 0; i < k.n_layers; ++i) {
        const LayerGraph& g = k.graph[i];
        if (g.n_in < 1 || g.n_in > 2) return false;
        int cols = 0;
        for (int j = 0; j < g.n_in; ++j) {
            if (!input_ok(k.acts, g.in[j])) return false;
            cols += g.in[j].width();
            n_pos += g.in[j].is_pos();
            n_dir += g.in[j].is_dir();
        }
        if (cols != k.dims[i][1]) return false;
        if (g.da_region < 0 || g.da_region >= k.grads.n) return false;
        const int w = k.grads.width[g.da_region];
        if (g.da_c0 < 0 || g.da_c1 > w || g.da_c1 - g.da_c0 != k.dims[i][0]) return false;
        if (g.head ? (w != 4 || g.da_region != k.grads.n - 1) : (g.da_c0 != 0 || g.da_c1 != w)) return false;
    }
    return n_pos >= 1 && n_pos <= 2 && n_dir <= 1;
}
constexpr bool film_graphs_ok() {
    for (int L = kFilmDepthMin; L <= kFilmDepthMax; ++L)
        if (!graph_ok(make_film_kind(L, true)) || !graph_ok(make_film_kind(L, false))) return false;
    return true;
}
static_assert(graph_ok(kFieldKinds[MI_FIELD_NERF]) && graph_ok(kFieldKinds[MI_FIELD_SIREN_NERF]) &&
                  graph_ok(kFieldKinds[MI_FIELD_FILM_SIREN_NERF]) && graph_ok(kFieldKinds[MI_FIELD_FILM_SIREN_NERF_NODIR]) &&
                  graph_ok(kFieldKinds[MI_FIELD_TINY_NERF]) && film_graphs_ok(),
              "every kind's graph tiles its weights' columns out of regions of the right width");
// ... and the checks can fail: NeRF with one input moved
constexpr FieldKind nerf_with_input(int layer, int input, int region, int shift) {
    FieldKind k = kFieldKinds[MI_FIELD_NERF];
    LayerInput& in = k.graph[layer].in[input];
    in.region = region; in.c0 += shift; in.c1 += shift;
    return k;
}
static_assert(graph_ok(nerf_with_input(kSkipLayer, 1, 5, 0)), "the unchanged copy passes");
static_assert(!graph_ok(nerf_with_input(kSkipLayer, 1, 5, 1)), "skip layer: second input shifted by one column");
static_assert(!graph_ok(nerf_with_input(9, 1, 11, 0)) && !graph_ok(nerf_with_input(9, 1, 0, 0)), "dir layer: wrong region for E_dir");

// ---- the packed streams against the graph ----------------------------------------------------------------------------
// Forward: one segment (field_layout.h) per non-head layer, in layer order: the layer's bias first, then the three weight
// columns of each K = 3 (xin) input, then whole heads (a head's rows in order, then its scalars); its K blocks are the
// layer's other inputs in 32-wide blocks, each as many row blocks high as the layer has outputs.
constexpr bool fwd_segments_ok(const FieldKind& k) {
    const Segments S = segments(k.fwd);
    if (S.covered != k.fwd.n_items) return false;
    int layer = -1;
    for (int i = 0; i < S.n; ++i) {
        const Segment& s = S.seg[i];
        if (s.layer <= layer || s.layer >= k.n_layers || k.graph[s.layer].head || s.aux > kMaxAuxPieces) return false;
        layer = s.layer;
        const LayerGraph& g = k.graph[layer];
        if (s.piece(AUX_BIAS, layer) != 0) return false;
        int a = 1, kb = 0;
        for (int j = 0, wcol = 0; j < g.n_in; wcol += g.in[j++].width()) {
            if (g.in[j].cls != SRC_XIN) { kb += (g.in[j].width() + 31) / 32; continue; }
            for (int c = 0; c < 3; ++c)
                if (s.piece(AUX_WCOL, layer, wcol + c) != a++) return false;
        }
        if (s.blocks != kb || (kb && s.mb * 32 != k.dims[layer][0])) return false;
        while (a < s.aux) {
            const int hl = s.item[a].layer;
            if (hl >= k.n_layers || !k.graph[hl].head) return false;
            for (int r = 0; r < k.dims[hl][0]; ++r)
                if (s.piece(AUX_WROW, hl, r) != a++) return false;
            if (s.piece(AUX_SCALARS, hl) != a++) return false;
        }
        if (a != s.aux) return false;
    }
    return S.n == k.n_layers - 2;
}
// Backward chain: one segment per non-head layer but the first, in reverse layer order: head rows only in front of the K
// blocks, which are the layer's outputs in 32-wide blocks for the 256 rows of its hidden input; every head row once.
constexpr bool bwd_segments_ok(const FieldKind& k) {
    const Segments S = segments(k.bwd);
    if (S.covered != k.bwd.n_items) return false;
    int layer = k.n_layers, rows = 0;
    for (int i = 0; i < S.n; ++i) {
        const Segment& s = S.seg[i];
        if (s.layer >= layer || s.layer < 1 || k.graph[s.layer].head || s.aux > kMaxAuxPieces) return false;
        layer = s.layer;
        if (s.blocks * 32 != k.dims[layer][0] || s.mb * 32 != kHidden) return false;
        for (int a = 0; a < s.aux; ++a) {
            const AuxItem& it = s.item[a];
            if (it.kind != AUX_WROW || !k.graph[it.layer].head || it.index >= k.dims[it.layer][0] || s.piece(AUX_WROW, it.layer, it.index) != a)
                return false;
            ++rows;
        }
    }
    return S.n == k.n_layers - 3 && rows == k.dims[k.sigma_head][0] + k.dims[k.rgb_head()][0];
}
constexpr bool segments_ok(const FieldKind& k) { return fwd_segments_ok(k) && bwd_segments_ok(k); }
// The run-time-depth FiLM kernels take their shapes from depth 8: at every depth the segments at the same distance from
// either end of the stream (forward: two from the front, three from the back; backward: one and one) have depth 8's
// shapes, and every segment between has the shape of depth 8's.
constexpr bool film_depth_like_8(int L, bool use_dir, bool bwd) {
    const FieldKind k = make_film_kind(L, use_dir), k8 = make_film_kind(8, use_dir);
    const Segments S = segments(bwd ? k.bwd : k.fwd), D = segments(bwd ? k8.bwd : k8.fwd);
    const int front = bwd ? 1 : 2, back = bwd ? 1 : 3;
    if (S.n != (bwd ? L : L + 1) || D.n != (bwd ? 8 : 9) || k.sigma_segments() != L) return false;
    for (int i = 0; i < S.n; ++i) {
        const Segment& d = i < front ? D.seg[i] : S.n - i <= back ? D.seg[D.n - (S.n - i)] : D.seg[front];
        if (!S.seg[i].same_shape(d)) return false;
    }
    return D.uniform(1, D.n - (bwd ? 2 : 4));       // the kernels' hidden-layer loops at depth 8
}
constexpr bool film_segments_ok(bool use_dir) {
    for (int L = kFilmDepthMin; L <= kFilmDepthMax; ++L)
        if (!segments_ok(make_film_kind(L, use_dir)) || !film_depth_like_8(L, use_dir, false) || !film_depth_like_8(L, use_dir, true))
            return false;
    return true;
}
static_assert(segments_ok(kFieldKinds[MI_FIELD_NERF]) && segments_ok(kFieldKinds[MI_FIELD_SIREN_NERF]) &&
                  segments_ok(kFieldKinds[MI_FIELD_FILM_SIREN_NERF]) && segments_ok(kFieldKinds[MI_FIELD_FILM_SIREN_NERF_NODIR]) &&
                  segments_ok(kFieldKinds[MI_FIELD_TINY_NERF]) && film_segments_ok(true) && film_segments_ok(false),
              "every kind's streams carry, segment by segment, what its graph's layers consume");
// ... and the checks can fail: NeRF's forward stream with the sigma head's row in front of layers_pos.7's bias, and with
// layers_pos.3 one K block short
constexpr FieldKind nerf_fwd_with(int segment, int at, bool swap) {
    FieldKind k = kFieldKinds[MI_FIELD_NERF];
    const int i = segments(k.fwd).seg[segment].first + at;
    if (swap) {                               // items i and i + 1 trade places (both are one piece: the offsets stay)
        const PackItem t = k.fwd.item[i];
        k.fwd.item[i] = k.fwd.item[i + 1];
        k.fwd.item[i + 1] = t;
    } else if (at >= 0) {                     // item i leaves
        for (int j = i; j + 1 < k.fwd.n_items; ++j) { k.fwd.item[j] = k.fwd.item[j + 1]; k.fwd.dst_off[j] = k.fwd.dst_off[j + 1]; }
        --k.fwd.n_items;
    }
    return k;
}
static_assert(segments_ok(nerf_fwd_with(7, -1, false)), "the unchanged copy passes");
static_assert(!segments_ok(nerf_fwd_with(7, 0, true)), "a head row in front of its layer's bias");
static_assert(!segments_ok(nerf_fwd_with(3, 1, false)), "a layer's K blocks one short");
static_assert(nerf_acts().relu_switch0() == 12 && tiny_acts().relu_switch0() == 7 && siren_acts().relu_switch0() < 0,
              "the ReLU kinds' switch regions follow their layer inputs");

// ---- MI_FIELD_FILM_DEPTH kinds -------------------------------------------------------------------------------------
// A depth kind is no row of kFieldKinds and has no table in constant memory (adam_step.hip keeps one PackTable pair per
// fixed kind there, about 11 KB each; eighteen more do not fit in 64 KB).  The host reads a depth kind's descriptor from
// field_kind() (field_kinds_host.h); the kernels take the depth as a run-time argument and compute stream items with film_item().
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

}  // namespace mi
