// The wave kernels' __global__ wrappers and their launch path, shared by the translation units that instantiate them.
//
// k_wave_g: several envs per wavefront (sfl_wave.h run_groups), G lanes per env, SFL_GROUP_BLOCK / G envs per
// block.  k_wave / k_wave2: one env per wavefront (sfl_wave.h run).  Which unit compiles which kernel: owner()
// below -- variant 7 (the bench's c3 shape) in sfl_kwave_v7.hip with the register-minimising scheduler, the
// HPG = true kernels (hyperparameter groups, sfl_set_hparam_groups: the plain launch of every shape) in
// sfl_kwave_hpg.hip and -- variant 7 -- sfl_kwave_hpg_v7.hip, the EXT = true kernels (external-action mode,
// sfl_env_begin_wave) in sfl_kwave_ext.hip, the BANK = true kernels (policy-bank evaluation, sfl_bank_eval) in
// sfl_kwave_bank.hip, so that they compile in parallel with sfl.hip, which has all the others.
//
// Waves per SIMD the grouped kernel is register-budgeted for (sfl::kVariants[v].OCC): shapes with one train
// slot per lane (TW <= G) 4 -- c2 (variant 6): 918 M vs 805 M at 3 (VGPR-bound, spills a little; 5: 589 M) --,
// two slots per lane 4 with the prefetch ring (SFL_PF_RING: the LDS then allows 4 blocks per CU), 3 without it.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

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
// EXT: external-action mode's env step (sfl_env_begin_wave; WEnv::ext_run), one decision per launch
template <int PPL, int SPL, int TW, bool TRACE, bool TIMED = false, bool HPG = false, bool EXT = false>
__global__ void __launch_bounds__(SFL_WAVE_BLOCK) __attribute__((amdgpu_waves_per_eu(SFL_WAVE_OCC))) k_wave(const sfl::SflMap* __restrict__ m, const sfl::SflState* __restrict__ s,
                                              const sfl::SflCtl* __restrict__ c) {
  sfl::wave::run<PPL, SPL, TW, TRACE, false, TIMED, HPG, EXT>(*m, *s, *c);
}
template <int PPL, int SPL, int TW, bool TRACE, bool TIMED = false, bool HPG = false, bool EXT = false>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SFL_WAVE2_OCC))) k_wave2(const sfl::SflMap* __restrict__ m,
                                                                                   const sfl::SflState* __restrict__ s,
                                                                                   const sfl::SflCtl* __restrict__ c) {
  sfl::wave::run<PPL, SPL, TW, TRACE, false, TIMED, HPG, EXT>(*m, *s, *c);
}

template <int PPL, int SPL, int TW, bool TRACE, int G, int OCC, bool TIMED = false, bool LM = false, bool HPG = false, bool EXT = false>
__global__ void __launch_bounds__(SFL_GROUP_BLOCK) __attribute__((amdgpu_waves_per_eu(OCC)))
k_wave_g(const sfl::SflMap* __restrict__ m, const sfl::SflState* __restrict__ s, const sfl::SflCtl* __restrict__ c) {
  sfl::wave::run_groups<PPL, SPL, TW, TRACE, G, TIMED, LM, HPG, EXT>(*m, *s, *c);
}

// BANK: policy-bank evaluation (sfl_bank_eval; sfl_wave.h BANK): one greedy episode per env on a table of the handle's
// read-only bank.  Kernels of their own names with the shape's arguments only (no trace, no timers, no groups), so the
// existing kernels keep their symbols; the same launch bounds and register budgets as the shape's other kernels.
template <int PPL, int SPL, int TW>
__global__ void __launch_bounds__(SFL_WAVE_BLOCK) __attribute__((amdgpu_waves_per_eu(SFL_WAVE_OCC)))
k_wave_bank(const sfl::SflMap* __restrict__ m, const sfl::SflState* __restrict__ s, const sfl::SflCtl* __restrict__ c) {
  sfl::wave::run<PPL, SPL, TW, false, false, false, false, false, true>(*m, *s, *c);
}
template <int PPL, int SPL, int TW>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SFL_WAVE2_OCC)))
k_wave2_bank(const sfl::SflMap* __restrict__ m, const sfl::SflState* __restrict__ s, const sfl::SflCtl* __restrict__ c) {
  sfl::wave::run<PPL, SPL, TW, false, false, false, false, false, true>(*m, *s, *c);
}
template <int PPL, int SPL, int TW, int G, int OCC, bool LM>
__global__ void __launch_bounds__(SFL_GROUP_BLOCK) __attribute__((amdgpu_waves_per_eu(OCC)))
k_wave_g_bank(const sfl::SflMap* __restrict__ m, const sfl::SflState* __restrict__ s, const sfl::SflCtl* __restrict__ c) {
  sfl::wave::run_groups<PPL, SPL, TW, false, G, false, LM, false, false, true>(*m, *s, *c);
}

// BANK with a recording armed (sfl_bank_record; sfl_wave.h REC): kernels of their own again, launched only while a
// recording is armed, so that the evaluation without one runs the kernels above unchanged
template <int PPL, int SPL, int TW>
__global__ void __launch_bounds__(SFL_WAVE_BLOCK) __attribute__((amdgpu_waves_per_eu(SFL_WAVE_OCC)))
k_wave_bank_rec(const sfl::SflMap* __restrict__ m, const sfl::SflState* __restrict__ s, const sfl::SflCtl* __restrict__ c) {
  sfl::wave::run<PPL, SPL, TW, false, false, false, false, false, true, true>(*m, *s, *c);
}
template <int PPL, int SPL, int TW>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SFL_WAVE2_OCC)))
k_wave2_bank_rec(const sfl::SflMap* __restrict__ m, const sfl::SflState* __restrict__ s, const sfl::SflCtl* __restrict__ c) {
  sfl::wave::run<PPL, SPL, TW, false, false, false, false, false, true, true>(*m, *s, *c);
}
template <int PPL, int SPL, int TW, int G, int OCC, bool LM>
__global__ void __launch_bounds__(SFL_GROUP_BLOCK) __attribute__((amdgpu_waves_per_eu(OCC)))
k_wave_g_bank_rec(const sfl::SflMap* __restrict__ m, const sfl::SflState* __restrict__ s, const sfl::SflCtl* __restrict__ c) {
  sfl::wave::run_groups<PPL, SPL, TW, false, G, false, LM, false, false, true, true>(*m, *s, *c);
}

// SCHED: handles with a seed schedule (sfl_set_seed_schedule; sfl_wave.h SCHED): the plain, the HPG and the EXT launch
// of every shape, again as kernels of their own names, so that every other handle runs the kernels it ran before
template <int PPL, int SPL, int TW, bool HPG, bool EXT>
__global__ void __launch_bounds__(SFL_WAVE_BLOCK) __attribute__((amdgpu_waves_per_eu(SFL_WAVE_OCC)))
k_wave_sched(const sfl::SflMap* __restrict__ m, const sfl::SflState* __restrict__ s, const sfl::SflCtl* __restrict__ c) {
  sfl::wave::run<PPL, SPL, TW, false, false, false, HPG, EXT, false, false, true>(*m, *s, *c);
}
template <int PPL, int SPL, int TW, bool HPG, bool EXT>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SFL_WAVE2_OCC)))
k_wave2_sched(const sfl::SflMap* __restrict__ m, const sfl::SflState* __restrict__ s, const sfl::SflCtl* __restrict__ c) {
  sfl::wave::run<PPL, SPL, TW, false, false, false, HPG, EXT, false, false, true>(*m, *s, *c);
}
template <int PPL, int SPL, int TW, int G, int OCC, bool LM, bool HPG, bool EXT>
__global__ void __launch_bounds__(SFL_GROUP_BLOCK) __attribute__((amdgpu_waves_per_eu(OCC)))
k_wave_g_sched(const sfl::SflMap* __restrict__ m, const sfl::SflState* __restrict__ s, const sfl::SflCtl* __restrict__ c) {
  sfl::wave::run_groups<PPL, SPL, TW, false, G, false, LM, HPG, EXT, false, false, true>(*m, *s, *c);
}

// ---- one launch path from the shape table ---------------------------------------------------------------------
// A cell = a row v of sfl::kVariants (1 .. kNumVariants - 1) x a launch mode.  Everything about a cell follows from
// the row: its kernel family, its grid and block, and the translation unit that compiles it.
static_assert(sizeof(sfl::kVariants) / sizeof(sfl::kVariants[0]) == sfl::kNumVariants, "kNumVariants counts kVariants' rows");
// Hpg: a handle with hyperparameter groups (plain only); Ext: a handle in external-action mode on the wave kernels
// (sfl_env_begin_wave) -- every row but the LM one, whose handles step the same shape without the LDS tables;
// Bank: an evaluation handle's episode launch (sfl_bank_eval) -- every row, the LM one with a cell of its own (a
// launch is a whole episode, hundreds of decisions per env, which is what the copy of the tables into LDS pays for;
// external-action mode's single decision per launch is not)
// BankRec: the same launch with a recording armed (sfl_bank_record): every row again
// Sched / SchedHpg / SchedExt: Plain / Hpg / Ext on a handle with a seed schedule (sfl_set_seed_schedule)
enum class Mode { Plain, Trace, Timed, Hpg, Ext, Bank, BankRec, Sched, SchedHpg, SchedExt };
// libsfl.so's translation units (build.TUS): sfl.hip, sfl_kwave_v7.hip, sfl_kwave_hpg.hip, sfl_kwave_hpg_v7.hip,
// sfl_kwave_ext.hip, sfl_kwave_bank.hip, sfl_kwave_sched.hip, sfl_kwave_sched_hpg.hip, sfl_kwave_sched_v7.hip,
// sfl_kwave_sched_ext.hip
enum class Unit { Main, V7, Hpg, HpgV7, Ext, Bank, Sched, SchedHpg, SchedV7, SchedExt };
constexpr int kSchedVariant = 7;  // the bench's c3 shape: its units are built with the register-minimising scheduler
// the unit that owns a cell: it alone instantiates the cell's kernel, with its own compiler flags.  Every cell has
// exactly one owner (this function's value); a unit that does not define its launch_unit fails the link.
constexpr Unit owner(int v, Mode md) {
  if (md == Mode::Ext) return Unit::Ext;
  if (md == Mode::SchedExt) return Unit::SchedExt;
  if (md == Mode::Sched || md == Mode::SchedHpg)  // (variant 7's two: one unit with variant 7's scheduler)
    return v == kSchedVariant ? Unit::SchedV7 : md == Mode::Sched ? Unit::Sched : Unit::SchedHpg;
  if (md == Mode::Bank || md == Mode::BankRec) return Unit::Bank;
  if (md == Mode::Hpg) return v == kSchedVariant ? Unit::HpgV7 : Unit::Hpg;
  return v == kSchedVariant ? Unit::V7 : Unit::Main;
}
struct Launch {
  int variant;
  Mode mode;
  uint32_t E;
  hipStream_t stream;
  const sfl::SflMap* m;
  const sfl::SflState* s;
  const sfl::SflCtl* c;
};
// grid and block of row w's kernels (the partitioned local step's too): k_wave packs SFL_WAVE_BLOCK / 64 envs into a
// block, k_wave2 runs one env per 64-thread block, k_wave_g SFL_GROUP_BLOCK / G envs per block
constexpr bool two_slot(const sfl::WaveShape& w) { return w.G == 64 && w.TW > 64; }
constexpr unsigned block_of(const sfl::WaveShape& w) { return w.G < 64 ? SFL_GROUP_BLOCK : two_slot(w) ? 64 : SFL_WAVE_BLOCK; }
constexpr unsigned grid_of(const sfl::WaveShape& w, uint32_t E) {
  return two_slot(w) ? E : (unsigned)(((size_t)E * w.G + block_of(w) - 1) / block_of(w));
}
// launches cell (V, MD) if the launch asks for it and unit U owns it (only then is the kernel instantiated here)
template <Unit U, int V, Mode MD>
inline void launch_cell(const Launch& l) {
  if constexpr (owner(V, MD) == U) {
    constexpr sfl::WaveShape w = sfl::kVariants[V];
    constexpr bool TRACE = MD == Mode::Trace, TIMED = MD == Mode::Timed, HPG = MD == Mode::Hpg || MD == Mode::SchedHpg;
    constexpr bool EXT = MD == Mode::Ext || MD == Mode::SchedExt;
    constexpr bool SCHED = MD == Mode::Sched || MD == Mode::SchedHpg || MD == Mode::SchedExt;
    if (l.variant != V || l.mode != MD) return;
    if constexpr (SCHED) {
      if constexpr (EXT && w.LM)
        return;  // (no such cell: ext_variant maps the row to its twin)
      else if constexpr (w.G < 64)
        k_wave_g_sched<w.PPL, w.SPL, w.TW, w.G, w.OCC, (bool)w.LM, HPG, EXT><<<grid_of(w, l.E), block_of(w), 0, l.stream>>>(l.m, l.s, l.c);
      else if constexpr (two_slot(w))
        k_wave2_sched<w.PPL, w.SPL, w.TW, HPG, EXT><<<grid_of(w, l.E), block_of(w), 0, l.stream>>>(l.m, l.s, l.c);
      else
        k_wave_sched<w.PPL, w.SPL, w.TW, HPG, EXT><<<grid_of(w, l.E), block_of(w), 0, l.stream>>>(l.m, l.s, l.c);
    } else if constexpr (MD == Mode::Bank) {
      if constexpr (w.G < 64)
        k_wave_g_bank<w.PPL, w.SPL, w.TW, w.G, w.OCC, (bool)w.LM><<<grid_of(w, l.E), block_of(w), 0, l.stream>>>(l.m, l.s, l.c);
      else if constexpr (two_slot(w))
        k_wave2_bank<w.PPL, w.SPL, w.TW><<<grid_of(w, l.E), block_of(w), 0, l.stream>>>(l.m, l.s, l.c);
      else
        k_wave_bank<w.PPL, w.SPL, w.TW><<<grid_of(w, l.E), block_of(w), 0, l.stream>>>(l.m, l.s, l.c);
    } else if constexpr (MD == Mode::BankRec) {
      if constexpr (w.G < 64)
        k_wave_g_bank_rec<w.PPL, w.SPL, w.TW, w.G, w.OCC, (bool)w.LM><<<grid_of(w, l.E), block_of(w), 0, l.stream>>>(l.m, l.s, l.c);
      else if constexpr (two_slot(w))
        k_wave2_bank_rec<w.PPL, w.SPL, w.TW><<<grid_of(w, l.E), block_of(w), 0, l.stream>>>(l.m, l.s, l.c);
      else
        k_wave_bank_rec<w.PPL, w.SPL, w.TW><<<grid_of(w, l.E), block_of(w), 0, l.stream>>>(l.m, l.s, l.c);
    } else if constexpr (EXT && w.LM)
      return;  // (no such cell: ext_variant maps the row to its twin)
    else if constexpr (w.G < 64)
      k_wave_g<w.PPL, w.SPL, w.TW, TRACE, w.G, w.OCC, TIMED, (bool)w.LM, HPG, EXT><<<grid_of(w, l.E), block_of(w), 0, l.stream>>>(l.m, l.s, l.c);
    else if constexpr (two_slot(w))
      k_wave2<w.PPL, w.SPL, w.TW, TRACE, TIMED, HPG, EXT><<<grid_of(w, l.E), block_of(w), 0, l.stream>>>(l.m, l.s, l.c);
    else
      k_wave<w.PPL, w.SPL, w.TW, TRACE, TIMED, HPG, EXT><<<grid_of(w, l.E), block_of(w), 0, l.stream>>>(l.m, l.s, l.c);
  }
}
template <Unit U, int... I>
inline void launch_owned(const Launch& l, std::integer_sequence<int, I...>) {
  ((launch_cell<U, I + 1, Mode::Plain>(l), launch_cell<U, I + 1, Mode::Trace>(l), launch_cell<U, I + 1, Mode::Timed>(l),
    launch_cell<U, I + 1, Mode::Hpg>(l), launch_cell<U, I + 1, Mode::Ext>(l), launch_cell<U, I + 1, Mode::Bank>(l),
    launch_cell<U, I + 1, Mode::BankRec>(l), launch_cell<U, I + 1, Mode::Sched>(l), launch_cell<U, I + 1, Mode::SchedHpg>(l),
    launch_cell<U, I + 1, Mode::SchedExt>(l)), ...);
}
// a unit's launches: declared here, defined (SFL_KWAVE_UNIT) in the unit itself
template <Unit U>
void launch_unit(const Launch& l);
template <>
void launch_unit<Unit::Main>(const Launch& l);
template <>
void launch_unit<Unit::V7>(const Launch& l);
template <>
void launch_unit<Unit::Hpg>(const Launch& l);
template <>
void launch_unit<Unit::HpgV7>(const Launch& l);
template <>
void launch_unit<Unit::Ext>(const Launch& l);
template <>
void launch_unit<Unit::Bank>(const Launch& l);
template <>
void launch_unit<Unit::Sched>(const Launch& l);
template <>
void launch_unit<Unit::SchedHpg>(const Launch& l);
template <>
void launch_unit<Unit::SchedV7>(const Launch& l);
template <>
void launch_unit<Unit::SchedExt>(const Launch& l);
#define SFL_KWAVE_UNIT(U)                                                                           \
  template <>                                                                                       \
  void sflk::launch_unit<sflk::Unit::U>(const sflk::Launch& l) {                                    \
    sflk::launch_owned<sflk::Unit::U>(l, std::make_integer_sequence<int, sfl::kNumVariants - 1>{}); \
  }
// the launch of a cell, from any unit: handed to its owner
inline void launch(const Launch& l) {
  switch (owner(l.variant, l.mode)) {
    case Unit::Main: return launch_unit<Unit::Main>(l);
    case Unit::V7: return launch_unit<Unit::V7>(l);
    case Unit::Hpg: return launch_unit<Unit::Hpg>(l);
    case Unit::HpgV7: return launch_unit<Unit::HpgV7>(l);
    case Unit::Ext: return launch_unit<Unit::Ext>(l);
    case Unit::Bank: return launch_unit<Unit::Bank>(l);
    case Unit::Sched: return launch_unit<Unit::Sched>(l);
    case Unit::SchedHpg: return launch_unit<Unit::SchedHpg>(l);
    case Unit::SchedV7: return launch_unit<Unit::SchedV7>(l);
    case Unit::SchedExt: return launch_unit<Unit::SchedExt>(l);
  }
}

}  // namespace sflk
