/*
 * mi_render_kinds.h - the status codes and the field-kind ids of libmirender.so's C ABI, each stated once.  mi_render.h
 * includes it: a host of the ABI includes mi_render.h alone and ships both files.  The library's kernel units include this
 * file only, so an edit of an entry point's declaration does not reach them.
 */
#ifndef MI_RENDER_KINDS_H
#define MI_RENDER_KINDS_H

#define MI_OK 0
#define MI_EINVAL (-1)   /* bad argument (shape, kind, null pointer) */
#define MI_EHIP (-2)     /* HIP runtime error at launch */
#define MI_ERANGE (-3)   /* marching cubes: level outside [min, max] of the volume */

/* Field MLP kinds (state-dict layouts: SURVEY.md §8a a6-a8). */
#define MI_FIELD_NERF 0                   /* nerf/nerf.py:52-94   NeRF            */
#define MI_FIELD_SIREN_NERF 1             /* nerf/nerf.py:120-170 SirenNeRF       */
#define MI_FIELD_FILM_SIREN_NERF 2        /* pi_GAN/modules.py:70-118 use_dir=True  */
#define MI_FIELD_FILM_SIREN_NERF_NODIR 3  /* pi_GAN/modules.py:70-118 use_dir=False */
#define MI_FIELD_TINY_NERF 4              /* build-defined 4-layer net for BASELINE C1 */
#define MI_FIELD_KINDS 5                  /* the fixed kinds above */
/* FilmSirenNeRF(hidden_dim=256, hidden_layers=L, use_dir) for any MI_FIELD_FILM_DEPTH_MIN <= L <= MI_FIELD_FILM_DEPTH_MAX
 * (pi_GAN/modules.py:73): a kind id outside the fixed kinds, accepted by every entry point that takes a `kind`.  Its state
 * dict is input_layer, hidden_layers.0 .. L-2, output_layer_sigma.0, hidden_layer_rgb, output_layer_rgb.0 (L + 3 linear
 * layers) and its FiLM table has mi_field_film_layers(kind) = L + 1 rows.  L = 8 is the network of kinds 2 / 3 and gives
 * the same bits.  A depth outside the range is MI_EINVAL. */
#define MI_FIELD_FILM_DEPTH_MIN 4
#define MI_FIELD_FILM_DEPTH_MAX 12
#define MI_FIELD_FILM_DEPTH(hidden_layers, use_dir) (0x100 + 2 * (hidden_layers) + ((use_dir) ? 1 : 0))

#endif /* MI_RENDER_KINDS_H */
