// Variant 7 of k_wave_g (the c3 shape) for handles with hyperparameter groups (HPG = true), built like
// sfl_kwave_v7.hip with the register-minimising machine scheduler (build.TUS).
#include "sfl_kwave_g.h"

namespace sflk {
static_assert(sfl::kVariants[kSchedVariant].G == 16 && sfl::kVariants[kSchedVariant].TW == 32, "variant 7 is the c3 shape");
}
SFL_KWAVE_UNIT(HpgV7)
