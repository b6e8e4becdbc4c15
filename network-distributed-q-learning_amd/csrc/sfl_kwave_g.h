// The wave kernels' __global__ wrappers, shared by the translation units that instantiate them.
//
// k_wave_g: several envs per wavefront (sfl_wave.h run_groups), G lanes per env, SFL_GROUP_BLOCK / G envs per
// block: sfl.hip (every shape but variant 7) and sfl_kwave_v7.hip (variant 7, the bench's c3 shape, compiled with
// the register-minimising scheduler).  k_wave / k_wave2: one env per wavefront (sfl_wave.h run): sfl.hip.
// HPG = true (hyperparameter groups, sfl_set_hparam_groups): the plain instantiation of every shape, in
// sfl_kwave_hpg.hip and -- variant 7, with variant 7's scheduler -- sfl_kwave_hpg_v7.hip, so that they compile in
// parallel with sfl.hip; sfl.hip only declares them (extern template).
//
// Waves per SIMD the grouped kernel is register-budgeted for (sfl::kVariants[v].OCC): shapes with one train
// slot per lane (TW <= G) 4 -- c2 (variant 6): 918 M vs 805 M at 3 (VGPR-bound, spills a little; 5: 589 M) --,
// two slots per lane 4 with the prefetch ring (SFL_PF_RING: the LDS then allows 4 blocks per CU), 3 without it.
#pragma once
#include <hip/hip_runtime.h>

#include "sfl_engine.h"
#include "sfl_wave.h"

#ifndef SFL_WAVE_OCC
#define SFL_WAVE_OCC 6  // waves per SIMD the one-env-per-wave kernel is register-budgeted for (6: 80 VGPRs)
#endif
// maps with 65-128 trains (two train slots per lane): one env per 64-thread block (its LDS is
// ~22 KB), register budget for the LDS-bound occupancy of 2 waves per SIMD
#ifndef SFL_WAVE2_OCC
#define SFL_WAVE2_OCC (SFL_PF_RING64 > 0 ? 4 : 2)  // waves per SIMD k_wave2 is register-budgeted for
#endif

namespace sflk {

// One env per wavefront (sfl_wave.h): 4 envs per block.  PPL / SPL = semaphore / counter
// registers per lane (sfl::kVariants).
// TIMED: the learn() / test() instantiation, with the sampled phase timers (sfl_wave.h PhaseTimer); the
// benchmark's sfl_step runs the untimed one
template <int PPL, int SPL, int TW, bool TRACE, bool TIMED = false, bool HPG = false>
__global__ void __launch_bounds__(SFL_WAVE_BLOCK) __attribute__((amdgpu_waves_per_eu(SFL_WAVE_OCC))) k_wave(const sfl::SflMap* __restrict__ m, const sfl::SflState* __restrict__ s,
                                              const sfl::SflCtl* __restrict__ c) {
  sfl::wave::run<PPL, SPL, TW, TRACE, false, TIMED, HPG>(*m, *s, *c);
}
template <int PPL, int SPL, int TW, bool TRACE, bool TIMED = false, bool HPG = false>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SFL_WAVE2_OCC))) k_wave2(const sfl::SflMap* __restrict__ m,
                                                                                   const sfl::SflState* __restrict__ s,
                                                                                   const sfl::SflCtl* __restrict__ c) {
  sfl::wave::run<PPL, SPL, TW, TRACE, false, TIMED, HPG>(*m, *s, *c);
}

template <int PPL, int SPL, int TW, bool TRACE, int G, int OCC, bool TIMED = false, bool LM = false, bool HPG = false>
__global__ void __launch_bounds__(SFL_GROUP_BLOCK) __attribute__((amdgpu_waves_per_eu(OCC)))
k_wave_g(const sfl::SflMap* __restrict__ m, const sfl::SflState* __restrict__ s, const sfl::SflCtl* __restrict__ c) {
  sfl::wave::run_groups<PPL, SPL, TW, TRACE, G, TIMED, LM, HPG>(*m, *s, *c);
}

// variant 7's three launches (traced, phase-timed, plain): explicit instantiation definitions in
// sfl_kwave_v7.hip, declarations (extern template) in sfl.hip
#define SFL_KWAVE_V7_ONE(PFX, TRACE, TIMED)                                                                        \
  PFX __global__ void k_wave_g<sfl::kVariants[7].PPL, sfl::kVariants[7].SPL, sfl::kVariants[7].TW, TRACE,           \
                               sfl::kVariants[7].G, sfl::kVariants[7].OCC, TIMED>(                                 \
      const sfl::SflMap* __restrict__, const sfl::SflState* __restrict__, const sfl::SflCtl* __restrict__);
#define SFL_KWAVE_V7(PFX)              \
  namespace sflk {                     \
  SFL_KWAVE_V7_ONE(PFX, true, false)   \
  SFL_KWAVE_V7_ONE(PFX, false, true)   \
  SFL_KWAVE_V7_ONE(PFX, false, false)  \
  }

// the grouped-hyperparameter (HPG) launch of variant v, plain only: explicit instantiation definitions in
// sfl_kwave_hpg.hip / sfl_kwave_hpg_v7.hip, declarations in sfl.hip
#define SFL_KARGS const sfl::SflMap* __restrict__, const sfl::SflState* __restrict__, const sfl::SflCtl* __restrict__
#define SFL_HPG_KW(PFX, v)                                                                                          \
  PFX __global__ void k_wave<sfl::kVariants[v].PPL, sfl::kVariants[v].SPL, sfl::kVariants[v].TW, false, false, true>( \
      SFL_KARGS);
#define SFL_HPG_KW2(PFX, v)                                                                                          \
  PFX __global__ void k_wave2<sfl::kVariants[v].PPL, sfl::kVariants[v].SPL, sfl::kVariants[v].TW, false, false, true>( \
      SFL_KARGS);
#define SFL_HPG_KG(PFX, v)                                                                                    \
  PFX __global__ void k_wave_g<sfl::kVariants[v].PPL, sfl::kVariants[v].SPL, sfl::kVariants[v].TW, false,      \
                               sfl::kVariants[v].G, sfl::kVariants[v].OCC, false, (bool)sfl::kVariants[v].LM, true>( \
      SFL_KARGS);
#define SFL_KWAVE_HPG(PFX) \
  namespace sflk {         \
  SFL_HPG_KW(PFX, 1)       \
  SFL_HPG_KW(PFX, 2)       \
  SFL_HPG_KW(PFX, 3)       \
  SFL_HPG_KW(PFX, 4)       \
  SFL_HPG_KW2(PFX, 5)      \
  SFL_HPG_KG(PFX, 6)       \
  SFL_HPG_KG(PFX, 8)       \
  SFL_HPG_KG(PFX, 9)       \
  SFL_HPG_KG(PFX, 10)      \
  SFL_HPG_KG(PFX, 11)      \
  }
#define SFL_KWAVE_HPG_V7(PFX) \
  namespace sflk {            \
  SFL_HPG_KG(PFX, 7)          \
  }

#ifdef SFL_PROFILE
// (tuning builds) variant 7's phase cycles, read and cleared -- they count into sfl_kwave_v7.hip's own g_prof
void kwave_v7_prof_take(unsigned long long* pr);
#endif

}  // namespace sflk
