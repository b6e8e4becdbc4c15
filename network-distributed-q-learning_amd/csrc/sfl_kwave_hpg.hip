// The wave kernels of handles with hyperparameter groups (sfl_set_hparam_groups; HPG = true in sfl_wave.h): the
// plain launch (no trace, no phase timers) of every shape but variant 7, in a translation unit of its own so that
// it compiles in parallel with sfl.hip.  Variant 7: sfl_kwave_hpg_v7.hip.  The unit's cells: sflk::owner, sfl_kwave_g.h.
#include "sfl_kwave_g.h"

SFL_KWAVE_UNIT(Hpg)
