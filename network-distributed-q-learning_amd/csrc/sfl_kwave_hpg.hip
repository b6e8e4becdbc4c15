// The wave kernels of handles with hyperparameter groups (sfl_set_hparam_groups; HPG = true in sfl_wave.h): the
// plain launch (no trace, no phase timers) of every shape but variant 7, in a translation unit of its own so that
// it compiles in parallel with sfl.hip.  Variant 7: sfl_kwave_hpg_v7.hip.
#include "sfl_kwave_g.h"

namespace sflk {
static_assert(sfl::kNumVariants == 12 && sfl::kVariants[5].TW > 64 && sfl::kVariants[4].G == 64 && sfl::kVariants[6].G < 64,
              "variants 1-4 are k_wave shapes, 5 the two-slot k_wave2 shape, 6-11 grouped");
}
SFL_KWAVE_HPG(template)
