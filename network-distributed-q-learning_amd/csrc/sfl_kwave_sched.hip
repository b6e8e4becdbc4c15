// The wave kernels of handles with a seed schedule (sfl_set_seed_schedule; SCHED = true in sfl_wave.h):
// the plain launch of every shape but variant 7.  A translation unit of its own, so that it compiles in parallel with sfl.hip.
// The unit's cells: sflk::owner, sfl_kwave_g.h.
#include "sfl_kwave_g.h"

SFL_KWAVE_UNIT(Sched)
