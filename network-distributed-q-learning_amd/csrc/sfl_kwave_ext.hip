// The wave kernels of external-action mode (sfl_env_begin_wave; EXT = true in sfl_wave.h): the env step of every
// shape but the LM one, one decision per launch, in a translation unit of its own so that it compiles in parallel
// with sfl.hip.  The unit's cells: sflk::owner, sfl_kwave_g.h.
#include "sfl_kwave_g.h"

SFL_KWAVE_UNIT(Ext)
