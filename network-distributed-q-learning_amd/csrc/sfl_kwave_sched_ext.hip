// The wave kernels of handles with a seed schedule (sfl_set_seed_schedule; SCHED = true in sfl_wave.h):
// external-action mode's env step of every shape but the LM one.  A translation unit of its own, so that it compiles in parallel with sfl.hip.
// The unit's cells: sflk::owner, sfl_kwave_g.h.
#include "sfl_kwave_g.h"

SFL_KWAVE_UNIT(SchedExt)
