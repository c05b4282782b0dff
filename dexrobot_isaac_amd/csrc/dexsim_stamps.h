// dexsim_stamps.h -- the per-wave cycle stamps of the profiling build (-DDEXSIM_PROFILE_PHASES, read by scripts/phase_profile.py):
// lane 0 of a wave writes "s_memtime since the start of the body" into a row of the arena field `crow`, which the fused step path
// leaves idle.  The product is never built with the flag: there Stamps is empty and every call is nothing.  Only this file tests it.
#pragma once
// The row map: (group, first row, rows per wave, slots, waves, bodies, detail); slot s of wave w in body b is row
// first + DEXSIM_PROFILE_BODY_ROWS * b + rows per wave * w + s.  waves: bit w = wave w stamps (0xff: every wave, 7 in the step kernels,
// 8 in k_post).  bodies: the bodies whose rows the group owns, 5 for what a sub-step body stamps (0: the single-body launch, 1-4: the
// bodies of k_physics4), 1 for the post block.  detail: 0 = in every profiling build, else the group's bit in
// -DDEXSIM_PROFILE_DETAIL=<group>[|<group>...] (default SWEEP05, NONE for none): a stamp inside a phase perturbs what it measures.
#define DEXSIM_PROFILE_BODY_ROWS 64
#define DEXSIM_PROFILE_GROUPS(X)                                                                                      \
  X(BODY, 0, 8, 8, 0xff, 5, 0)          /* phase boundaries of a sub-step body: BodySlot                            */ \
  X(POST, 320, 8, 4, 0xff, 1, 0)        /* post block, every wave: PostSlot                                         */ \
  X(POST_LOGIC, 384, 8, 5, 0x01, 1, 0)  /* post block, wave 0's logic (each half from its own start): PostLogicSlot */ \
  X(SWEEP05, 448, 8, 5, 0x21, 5, 1)     /* pass 2 of the general path's sweeps, waves 0 and 5: SweepSlot            */ \
  X(SCHUR, 768, 8, 6, 0x01, 5, 2)       /* inside wave 0's Schur phase: SchurSlot                                   */ \
  X(PH2, 1088, 8, 3, 0x22, 5, 4)        /* inside phase 2 of the general path, waves 1 and 5: Ph2Slot               */ \
  X(SWEEP_ALL, 1408, 8, 5, 0xff, 5, 8)  /* pass 2 of the general path's sweeps, every wave: SweepSlot               */
#ifndef DEXSIM_PROFILE_DETAIL
#define DEXSIM_PROFILE_DETAIL SWEEP05
#endif
#define X(name, first, per_wave, slots, waves, bodies, detail) SG_##name,
enum StampGroup { DEXSIM_PROFILE_GROUPS(X) SG_COUNT };
#undef X
enum BodySlot { PH_BASE_CHAIN, PH_1, PH_2, PH_3_ROWS, PH_4_SWEEPS, PH_5, PH_PUBLISH, PH_GENERAL_8 /* (general path; not stamped at present) */ };
enum SchurSlot { SCHUR_START, SCHUR_COMPOSITE, SCHUR_OWN_ROWS, SCHUR_TOKENS, SCHUR_S_TAUB, SCHUR_SOLVED };
enum Ph2Slot { PH2_NARROW, PH2_BARRIER, PH2_APPENDED };
enum SweepSlot { SW_START, SW_WORK, SW_BARRIER1, SW_REDUCED, SW_BARRIER2 };
enum PostSlot { POST_A, POST_B, POST_ROWS, POST_OBS };
enum PostLogicSlot { PL_TASK_OBS, PL_TERMINATION, PL_REWARD_TERMS, PL_REWARD_TABLE, PL_STATS };
namespace stamp_detail {
struct Group { int first, per_wave, slots, waves, bodies, detail; };
#define X(name, first, per_wave, slots, waves, bodies, detail) name = detail,
enum { NONE = 0, DEXSIM_PROFILE_GROUPS(X) };
#undef X
#define X(name, first, per_wave, slots, waves, bodies, detail) {first, per_wave, slots, waves, bodies, detail},
constexpr Group groups[SG_COUNT] = {DEXSIM_PROFILE_GROUPS(X)};
#undef X
constexpr int selected = DEXSIM_PROFILE_DETAIL;
// a group owns the rows [first, first + body rows * bodies): inside crow, shared with no other group (any set of detail groups combines)
constexpr bool map_ok() {
  for (int g = 0; g < SG_COUNT; g++) {
    const Group& a = groups[g];
    if (a.slots > a.per_wave || 8 * a.per_wave > DEXSIM_PROFILE_BODY_ROWS || a.first < 0 || a.first + DEXSIM_PROFILE_BODY_ROWS * a.bodies > DEXSIM_ROWS_crow) return false;
    for (int h = 0; h < g; h++)
      if (a.first < groups[h].first + DEXSIM_PROFILE_BODY_ROWS * groups[h].bodies && groups[h].first < a.first + DEXSIM_PROFILE_BODY_ROWS * a.bodies) return false;
  }
  return true;
}
static_assert(map_ok(), "stamp rows: outside crow, or two groups overlap");
}   // namespace stamp_detail
struct Stamps {
#ifdef DEXSIM_PROFILE_PHASES
  unsigned long long t0; int body;   // s_memtime at the start of the body; which body
  DI static Stamps begin(int body) { return {__builtin_amdgcn_s_memtime(), body}; }
  // slot `slot` of group G for the calling wave, whose role is `wv`: lane 0 writes the time since t0 into column `col`, its own env
  // (the caller's `e`; `blockIdx.x * 64` where `e` names the env of a work item's owner or the caller has none)
  template <StampGroup G, typename Col>
  DI void mark(const Arena& A, int N, int wv, Col col, int slot) const {
    constexpr stamp_detail::Group g = stamp_detail::groups[G];
    if ((g.detail != 0 && !(stamp_detail::selected & g.detail)) || (threadIdx.x & 63) != 0 || (g.waves != 0xff && !((g.waves >> wv) & 1))) return;
    A.crow[(size_t)(g.first + DEXSIM_PROFILE_BODY_ROWS * body + g.per_wave * wv + slot) * N + col] = __int_as_float((int)(__builtin_amdgcn_s_memtime() - t0));
  }
#else
  DI static Stamps begin(int) { return {}; }
  template <StampGroup G, typename Col>
  DI void mark(const Arena&, int, int, Col, int) const {}
#endif
};
