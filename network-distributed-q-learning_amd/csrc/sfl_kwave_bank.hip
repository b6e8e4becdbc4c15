// The wave kernels of policy-bank evaluation (sfl_bank_eval; BANK = true in sfl_wave.h): one greedy episode per env
// on a read-only table of the handle's bank, for every row of sfl::kVariants (the LM row included), in a translation
// unit of its own so that it compiles in parallel with sfl.hip.  The unit's cells: sflk::owner, sfl_kwave_g.h.
#include "sfl_kwave_g.h"

SFL_KWAVE_UNIT(Bank)
