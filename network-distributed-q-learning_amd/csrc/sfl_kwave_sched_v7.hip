// The wave kernels of handles with a seed schedule (sfl_set_seed_schedule; SCHED = true in sfl_wave.h):
// variant 7's plain and grouped launch, built with variant 7's
// scheduler.  A translation unit of its own, so that it compiles in parallel with sfl.hip.
// The unit's cells: sflk::owner, sfl_kwave_g.h.
#include "sfl_kwave_g.h"

SFL_KWAVE_UNIT(SchedV7)
