// field_mlp_instances.h - what the forward's host unit (field_mlp.hip) and its three kernel units share: the variants a
// kind's kernel is instantiated in, and each unit's rows of the instance table.  A row holds one kernel address per variant
// (null: no such instance), constant-initialised in the unit that defines the kernels.
#pragma once
#include "../../include/mi_render_kinds.h"
#include "mi_device.h"

namespace mi {

// Variants: the inference, the training (layer inputs saved), the sigma-only and the windowed sigma-only instance of the
// kind's kernel, then the two kernels of the deferred colour branch (NeRF, TinyNeRF): the trunk-and-spill instance and the
// colour-branch kernel, then the list-driven inference instance and the list-driven training instance (NeRF, SirenNeRF,
// TinyNeRF: the kinds an occupancy grid exists for).
enum FwdVariant : int { FWD_INFER = 0, FWD_SAVE, FWD_SIGMA, FWD_SIGMA_WINDOW, FWD_SPILL, FWD_COLOUR, FWD_LIST, FWD_LIST_SAVE, FWD_VARIANTS };

// argument block of the two deferred-colour kernels (field_mlp_nerf.hip): every other instance takes MlpArgs
struct DeferMlpArgs : MlpArgs { DeferArgs defer; };

extern const void* const kNerfRows[2][FWD_VARIANTS];    // field_mlp_nerf.hip: MI_FIELD_NERF, MI_FIELD_TINY_NERF
extern const void* const kSirenRow[1][FWD_VARIANTS];    // field_mlp_siren.hip: MI_FIELD_SIREN_NERF
// field_mlp_film.hip: MI_FIELD_FILM_SIREN_NERF, ..._NODIR, then the run-time-depth instances without / with the direction
extern const void* const kFilmRows[4][FWD_VARIANTS];

}  // namespace mi
