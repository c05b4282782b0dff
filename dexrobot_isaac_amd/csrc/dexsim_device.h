// dexsim_device.h -- device-side data layout and small math for the gfx950 kernels.
//
// Data layout in HBM: every per-env quantity is one *field* of the arena, stored SoA as [row][env]
// (env fastest).  A wavefront of 64 lanes = 64 consecutive envs, so every load/store of a field row is one
// fully coalesced 256-byte transaction.  Wave-uniform constants (hand model, config) live in one DevParams
// block that the compiler reads through the scalar cache (s_load), costing no VGPRs.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/dexsim.h"

// (type, name, rows) -- the arena contract.  Rows * num_envs 4-byte words each.
#define DEXSIM_FIELDS(X)                                                                                    \
  /* physics state (replaces PhysX-owned state behind gym.acquire_*_tensor) */                              \
  X(float, q, 26) X(float, qd, 26) X(float, targets, 26)                                                    \
  X(float, box_pos, 3) X(float, box_quat, 4) X(float, box_lin, 3) X(float, box_ang, 3)                      \
  X(float, box_mass, 1) X(float, box_mu, 1)                                                                 \
  /* compact L1 state read by the fused post-physics kernel */                                              \
  X(float, site_pose, 77) X(float, hand_vel, 6) X(float, cforce, 51) X(float, cf5, 15)                      \
  /* dynamics -> contact-solve interface (one sub-step) */                                                  \
  X(float, jframe, 156) X(float, ufree, 32) X(float, fac_finv, 60)                                          \
  X(float, fac_g, 120) X(int, ncontact, 1) X(float, cgeom, DEXSIM_KMAX * 8) X(int, ccode, DEXSIM_KMAX)      \
  X(float, crow, DEXSIM_KMAX * 3 * 28) X(float, crowq, DEXSIM_KMAX * 3 * 28 + 4) X(float, clam, DEXSIM_KMAX * 3) X(float, chdr, DEXSIM_KMAX * 8) X(float, cstage, 6 * NP_STAGE * 9)                                         \
  /* warm-start cache: per contact key one float4 (impulses of the previous sub-step, tag), [key][env][4]; wgen = the env's sub-step generation */ \
  X(float, wlam, DEXSIM_NWKEY * 4) X(int, wgen, 1) X(int, csplit, 1)                                         \
  /* L2 state (ActionProcessor / ObservationEncoder / task / RewardCalculator / TerminationManager) */      \
  X(float, active_prev_targets, 18) X(float, active_rule_targets, 18) X(float, prev_actions, 18)            \
  X(float, actions, 18) X(float, prev_dof_pos, 26)                                                          \
  X(float, contact_duration_steps, 5) X(float, prev_contact_binary, 5) X(int, episode_step, 1)              \
  X(int, success_duration_steps, 1) X(int, success_conditions_met, 1) X(int, current_stage, 1)              \
  X(int, just2, 1) X(int, just3, 1) X(float, time_in_stage, 1) X(float, stage_contact_duration, 1)          \
  X(float, initial_box_pos, 3)                                                                              \
  X(float, prev_finger_dof_vel, 20) X(float, prev_hand_vel, 3) X(float, prev_hand_ang_vel, 3)               \
  X(int, prev_contacts, 5)                                                                                  \
  X(int, episode_success, 1) X(int, episode_failure, 1) X(int, success_reason, DEXSIM_NUM_SUCC)             \
  X(int, failure_reason, DEXSIM_NUM_FAIL) X(int, crit_success, DEXSIM_NUM_SUCC)                             \
  X(int, crit_failure, DEXSIM_NUM_FAIL) X(int, term_success, 1) X(int, term_failure, 1)                     \
  X(int, term_timeout, 1)                                                                                   \
  X(float, obs_all, DEXSIM_OBS_ALL_DIM) X(float, rew_comp, DEXSIM_NUM_REWROWS) X(float, rew, 1)             \
  X(int, reset_flag, 1) X(int, reset_count, 1)

struct Arena {
#define X(type, name, rows) type* name;
  DEXSIM_FIELDS(X)
#undef X
};

// (name, layout) -- the *persistent* arena fields: what dexsim_save_state / dexsim_load_state / dexsim_copy_envs move for an env
// (the arena part of a state record, include/dexsim.h).  Layout ROWS = plain [row][env] words, QUAD = [quad][env][4] (one
// 16-byte access per lane and quad).  Type and row count come from DEXSIM_FIELDS (DEXSIM_ROWS_<name> below), so the two lists
// cannot drift apart: a name that is not an arena field does not compile.
//
// Every field of DEXSIM_FIELDS is listed except the hand-off scratch of ONE sub-step, whose first access in a sub-step is a
// write, or a read guarded by data written earlier in the same sub-step:
//   jframe, fac_g, fac_finv  written by the chain walk / factorisation of every finger and base wave before the row builder and
//                            the Schur phase read them back;
//   ufree                    every word written by the free-velocity pass (fingers, base, box: the box rows are zeroed when
//                            there is no box) before the solve reads it;
//   cstage, cgeom, ccode     the narrowphase stages and compacts the sub-step's manifold; readers index below the contact count
//                            (DL_NC in LDS, or ncontact written by the same sub-step in the staged kernels);
//   crow, crowq, clam, chdr  written per list entry k < nc by the row builder, read for k < nc only (crowq's always-zero quad row
//                            is never written: it is zero from dexsim_init_state on, in every instance);
//   csplit                   written next to ncontact by the narrowphase, read by the solve of the same sub-step.
// ncontact IS part of the record although the kernels rewrite it before they read it: it is observable after the last sub-step.
// A record is therefore defined at control-step boundaries (and at sub-step boundaries of the staged entry points) only; the
// k_dynamics -> k_solve hand-off of the stand-alone test kernels is deliberately not part of it.
#define DEXSIM_STATE_FIELDS(X)                                                                              \
  X(q, ROWS) X(qd, ROWS) X(targets, ROWS) X(box_pos, ROWS) X(box_quat, ROWS) X(box_lin, ROWS) X(box_ang, ROWS) \
  X(box_mass, ROWS) X(box_mu, ROWS) X(site_pose, ROWS) X(hand_vel, ROWS) X(cforce, ROWS) X(cf5, ROWS)       \
  X(ncontact, ROWS) X(wlam, QUAD) X(wgen, ROWS)                                                             \
  X(active_prev_targets, ROWS) X(active_rule_targets, ROWS) X(prev_actions, ROWS) X(actions, ROWS)          \
  X(prev_dof_pos, ROWS) X(contact_duration_steps, ROWS) X(prev_contact_binary, ROWS) X(episode_step, ROWS)  \
  X(success_duration_steps, ROWS) X(success_conditions_met, ROWS) X(current_stage, ROWS) X(just2, ROWS)     \
  X(just3, ROWS) X(time_in_stage, ROWS) X(stage_contact_duration, ROWS) X(initial_box_pos, ROWS)            \
  X(prev_finger_dof_vel, ROWS) X(prev_hand_vel, ROWS) X(prev_hand_ang_vel, ROWS) X(prev_contacts, ROWS)     \
  X(episode_success, ROWS) X(episode_failure, ROWS) X(success_reason, ROWS) X(failure_reason, ROWS)         \
  X(crit_success, ROWS) X(crit_failure, ROWS) X(term_success, ROWS) X(term_failure, ROWS)                   \
  X(term_timeout, ROWS) X(obs_all, ROWS) X(rew_comp, ROWS) X(rew, ROWS) X(reset_flag, ROWS)                 \
  X(reset_count, ROWS)

#define DEXSIM_LAYOUT_ROWS 0
#define DEXSIM_LAYOUT_QUAD 1

// GPTR: view a pointer as global-address-space.  Field pointers that were loaded from memory (P->arena) are generic
// to the compiler and would be accessed with FLAT instructions (vmcnt + lgkmcnt, aperture check); kernel-argument
// copies are already known to be global, for them the cast is a no-op.
#define GPTR(p) ((__attribute__((address_space(1))) __typeof__(*(p))*)(p))
#define FLD(f, r) GPTR(A.f)[(size_t)(r) * N + e]

// Quad layout (round 3): the per-finger factor hand-off -- fac_g (G_f, 24 words = 6 quads per finger), fac_finv (Fhat_f^-1 lower
// triangle, 10 words in 3 quads per finger) and the finger part of jframe (axes + origins of the finger's 4 joints, 24 words = 6
// quads per finger, behind the 36 row-layout words of the base joints) -- is stored [quad][env][4]: a lane moves four consecutive
// words with ONE 16-byte access.  G_f alone is written and read back by every finger wave in every sub-step: 48 memory instructions
// become 12; the row builder's 58 dependent scalar loads become 15.
#define FQ(field, quad) ((__attribute__((address_space(1))) f4*)(A.field) + ((size_t)(quad) * N + e))
#define JFRAME_FQ0 9   /* first quad of finger 0's joint frames in jframe (36 base-joint words come first) */
// the manifold (cgeom: 2 quads per list entry: p.xyz n.x | n.yz gap mu) and the narrowphase staging blocks (cstage: 2 quads per staged
// contact, 6 waves x 15; their codes as plain rows behind the 180 quads) are FQ fields too
#define NP_STAGE 20                     /* staged entries per narrowphase wave: <= 12 contacts of its three capsules + <= 8 joint-limit rows */
#define CSTAGE_CODE0 (6 * NP_STAGE * 8)

#define CROW_W 28 /* words per contact row: t6 jf4 St6 Fj4 d3 rxd3 Dinv pad */
// crowq: the rows of streamed hand contacts in the quad layout of the LDS row store ([quad][env] of float4, 21 quads per
// contact), followed by ONE always-zero quad row (index KMAX * 21) that lanes without the contact read instead

enum {   // DEXSIM_ROWS_<field>: row count of every arena field (for DEXSIM_STATE_FIELDS)
#define X(type, name, rows) DEXSIM_ROWS_##name = (rows),
  DEXSIM_FIELDS(X)
#undef X
};

// per-joint constants packed as one 128-byte record: a wave fetches everything it needs about joint j with two
// s_load_dwordx16 instead of ~12 scattered scalar loads (the base-chain walk was scalar-load-latency bound)
struct JC {
  float qoff[4], poff[3], axis[3], com[3], inertia[6];
  float mass, kp, kd, armature, lo, hi;
  float pad[7];
};
static_assert(sizeof(JC) == 128, "JC must be 128 bytes");

struct DevParams {
  DexSimConfig cfg;
  DexHandModel model;
  float h;           // sub-step
  float box_inv_I_k; // 6 / size^2 : inv inertia of a solid cube = box_inv_I_k / mass
  // closed form of the configuration-independent part of the base chain (joints 0-2 prismatic, joint 3 the first
  // revolute): world axes A_j, the constant part Oc_j of the origin of joint frame j, orientation of frame 3 at q3 = 0
  float base_A[4][3], base_Oc[4][3], base_Q3z[4];
  unsigned obs_div_magic; // ceil(2^32 / num_obs): idx / num_obs == umulhi(idx, magic) for idx < 2^16 (obs_buf flush)
  int inertia_diag;  // every finger link's inertia is diagonal in its joint frame (host-side check of the model): rotate_inertia_diag
  float hand_reach;  // bound on |x - o5| over every point x of every hand capsule, for any joint configuration
                     // (o5 = origin of the palm joint frame): the hand-level broadphase of substep_body
  int obs_col_row[DEXSIM_OBS_ALL_DIM]; // obs_buf column -> obs_all row (flattened policy_observation_keys)
  JC jc[DEXSIM_NJ];  // packed copy of the per-joint model constants
  Arena arena;       // field pointers (filled by dexsim_bind): kernels with long live ranges read them on demand
                     // through the scalar cache instead of pinning 110 SGPRs of by-value kernel arguments
};

// counters block (ints): reduction scratch + device-side control flags
// CNT_ANY_RESET holds a STEP STAMP, not a boolean: the post block of control step `stamp` (a host-side counter, handed to
// every kernel in ApiPtrs::stamp) stores `stamp` when some env must reset; gated launches run iff the word equals their
// stamp.  Nothing ever clears the word, so no launch both clears and sets it (round 1 cleared it in block 0 of the very
// launch whose other blocks set it: an unordered write/atomic pair on a control flag).
#define CNT_ANY_RESET 0
#define CNT_SUCC 1        /* [NUM_SUCC] */
#define CNT_FAIL 2        /* [NUM_FAIL] */
#define CNT_TERM_SUCCESS 8
#define CNT_TERM_FAILURE 9
#define CNT_TERM_TIMEOUT 10
#define CNT_NUM_RESETS 11
#define CNT_CONTACTS 16   /* [2], by stamp parity: sum of active contacts of the control step's main physics step (last
                             sub-step); word stamp&1 is accumulated and read by the step, the other word is cleared for the next */
#define CNT_HAND_CONTACTS 18 /* [2], same scheme: the hand/box and hand/ground contacts among them */
#define CNT_SPIN_TIMEOUT 20  /* diagnostic build -DDEXSIM_DEBUG_SPIN only: (site << 24 | seq) of an LDS token wait that ran into its bound */
#define CNT_PHYS_STEPS 13
#define CNT_CONSECUTIVE 14 /* persistent */
#define CNT_RC_FIRST 15    /* persistent: RewardCalculator lazy prev-state init pending */

// the API tensors and per-launch words the host hands to the kernels by value (filled by dexsim_bind and the dexsim_set_* calls)
struct ApiPtrs {
  float* obs_buf; float* rew_buf; uint8_t* reset_buf; int64_t* episode_step_count; int64_t* episode_length;
  float* dof_state; float* root_state; float* rigid_body_states; float* contact_forces_all; float* full_dof_targets;
  const float* reset_samples;
  uint8_t* masks; const float* raw_targets;
  float* stats; int* counters;
  // optional second destination of the step outputs (dexsim_set_step_sink): the caller's rollout-buffer slot, written by
  // the same flush as obs_buf / rew_buf / reset_buf so that collecting a rollout costs no extra launch
  float* sink_obs; float* sink_rew; uint8_t* sink_done;
  float* sink_stats;     // optional copy of the step's statistics block (dexsim_set_stats_sink): row t of the rollout's (T, DEXSIM_STAT_WORDS) tensor
  float* actions_copy;   // optional (N, num_actions) copy of the actions consumed by the step (dexsim_set_action_copy)
  int skip_obs_all;      // dexsim_set_obs_dict_mode(1): the post block does not flush the 392 obs_all rows (the SoA rows behind obs_dict);
                         // obs_buf -- the policy keys -- is unaffected
  unsigned* probe;       // optional phase probe (dexsim_set_phase_probe): 4 words per workgroup, accumulated shader-clock ticks --
                         // [0] phases 3 + 4 of the general contact path (rows + sweeps), [1] whole k_physics4 launches, [2] number of
                         // sub-steps that ran the general path, [3] phase 4 alone (the sweeps)
  int stamp;             // stamp of the current control step (see CNT_ANY_RESET)
};

// Coupling (constants.py:71-88): the DOFs that each of the 18 controls drives, in the reference's order, with their scales.
// Controls 0-5 drive the base DOFs 0-5.  Every index is a compile-time constant in the unrolled loops that read the table.
struct CouplingGroup { int n, dof[3]; float scale[3]; };
constexpr CouplingGroup kCoupling[18] = {
    {1, {0}, {1}}, {1, {1}, {1}}, {1, {2}, {1}}, {1, {3}, {1}}, {1, {4}, {1}}, {1, {5}, {1}},
    {1, {6}, {1}},                          // thumb spread
    {1, {7}, {1}},                          // thumb MCP
    {2, {8, 9}, {1, 1}},                    // thumb DIP
    {3, {10, 18, 22}, {1, 1, 2}},           // finger spread: r_f_joint5_1 (DOF 22) turns twice as far
    {1, {11}, {1}}, {2, {12, 13}, {1, 1}},  // index MCP, DIP
    {1, {15}, {1}}, {2, {16, 17}, {1, 1}},  // middle MCP, DIP
    {1, {19}, {1}}, {2, {20, 21}, {1, 1}},  // ring MCP, DIP
    {1, {23}, {1}}, {2, {24, 25}, {1, 1}},  // pinky MCP, DIP
};
constexpr int kHeldDof = 14;   // r_f_joint3_1 (middle spread): driven by no control, its target is held at 0

// ------------------------------------------------------------------------------------------------- math
typedef float f2 __attribute__((ext_vector_type(2)));   // maps onto the gfx950 packed-FP32 VALU ops
typedef float f4 __attribute__((ext_vector_type(4)));   // 16-byte global accesses
// 16-byte store to global memory (address-space 1: no FLAT instruction even when the pointer came from memory)
__device__ __forceinline__ void st4_global(float* p, f4 v) { *(__attribute__((address_space(1))) f4*)p = v; }
__device__ __forceinline__ void st4_global(float* p, float a, float b, float c, float d) { f4 v; v.x = a; v.y = b; v.z = c; v.w = d; st4_global(p, v); }

struct V3 { float x, y, z; };
struct Q4 { float x, y, z, w; };
struct S6 { float xx, yy, zz, xy, xz, yz; }; // symmetric 3x3
struct M3 { float m[9]; };

#define DI __device__ __forceinline__

// LDS tokens: the words through which the waves of a step-kernel workgroup hand over to one another between barriers (who posts,
// who waits: dexsim_physics.hip.inc).  `sh` is the kernel's `extern __shared__` base, `word` an index in floats.  The accesses are
// volatile AND typed as LDS: a volatile access through a generic pointer is left alone by the address-space inference and becomes
// a FLAT instruction (sc0 sc1, waited for with vmcnt(0) lgkmcnt(0)), which is neither ordered with the DS instructions around it
// nor cheap; these compile to one ds_read_b32 / ds_write_b32.  DS instructions of a wave execute in order, so "data, then
// token" on the posting side and "token, then data" on the waiting side need compiler barriers only.
typedef volatile __attribute__((address_space(3))) float lds_tok_f;
typedef volatile __attribute__((address_space(3))) int lds_tok_i;
DI int lds_tok_load(const float* sh, int word) { return __float_as_int(((const lds_tok_f*)sh)[word]); }
DI void lds_tok_store(float* sh, int word, int v) { ((lds_tok_f*)sh)[word] = __int_as_float(v); }
DI int lds_cnt_load(const float* sh, int word) { return ((const lds_tok_i*)sh)[word]; }   // a counter kept by LDS atomics

DI V3 v3(float x, float y, float z) { return {x, y, z}; }
DI V3 v3p(const float* p) { return {p[0], p[1], p[2]}; }
DI V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
DI V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
DI V3 operator*(float s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
DI V3& operator+=(V3& a, V3 b) { a.x += b.x; a.y += b.y; a.z += b.z; return a; }
DI V3& operator-=(V3& a, V3 b) { a.x -= b.x; a.y -= b.y; a.z -= b.z; return a; }
DI float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
DI V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
DI float norm(V3 a) { return sqrtf(dot(a, a)); }
// Range-unscaled reciprocal, division and square roots for the step path.  The operators `1.f / x`, `a / b`, sqrtf(x) and
// 1.f / sqrtf(x) compile (2.5 ulp forms, FP32 denormals on) to the same v_rcp_f32 / v_sqrt_f32 / v_rsq_f32 wrapped in frexp / ldexp
// range scaling that only matters when an operand or the result is denormal: 5, 8, 6 and 6 instructions instead of 1, 2, 1 and 1.
// Inside the stated range the helpers return the operators' bits (tests/test_range_unscaled_math.py sweeps every bit pattern);
// outside it they differ (denormals are flushed by the hardware instruction), so every call site states in one line why its
// operand is in range.  Sites that cannot say so keep the operator.  rsq_n has no caller yet (the only
// 1.f / sqrtf on the step path is spd_solve's clamped pivot, one instruction already); it is kept, and swept by the test, for later.
// A site whose operator this build compiles as the correctly rounded v_div_scale / v_div_fmas / v_div_fixup sequence (schur_comp, the
// solver's split factors) cannot go on a helper either: the last bit differs.
// Two rewrites of the optimiser would change bits and are kept out: div_n's product is not contracted into a following add (the
// operator's quotient is not either: its last instruction is the ldexp), and a root that a helper divides by is made opaque()
// first (sqrt_n does it itself), so that div_n(a, root) stays v_sqrt_f32 + v_rcp_f32 like the operators' sequence instead of
// becoming v_rsq_f32.
DI float opaque(float x) { asm("" : "+v"(x)); return x; }   // no instruction: the value's origin is hidden from the optimiser
// rcp_n: x and 1/x normal (2^-126 <= |x| <= 2^126)
DI float rcp_n(float x) { return __builtin_amdgcn_rcpf(x); }
// div_n: b and 1/b normal as for rcp_n; a anything finite as long as the quotient is zero or normal
DI float div_n(float a, float b) {
#pragma clang fp contract(off)
  return a * __builtin_amdgcn_rcpf(b);
}
// sqrt_n: x zero or normal (the operator has no Newton step in this build: one v_sqrt_f32, as here)
DI float sqrt_n(float x) { return opaque(__builtin_amdgcn_sqrtf(x)); }
// rsq_n: x and the result normal (for 1.f / sqrtf(x) where the root has no other use: the operators are one v_rsq_f32 there)
DI float rsq_n(float x) { return __builtin_amdgcn_rsqf(x); }
// mulr: a product that is rounded on its own -- never contracted into a neighbouring add.  The specialised chain forms (model
// structure, see base_chain) use it where the general expression rounds the surviving product before the next add.
DI float mulr(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
// norm_n: |a| for a vector that is exactly zero or of model scale (a capsule axis): dot(a, a) zero or normal
DI float norm_n(V3 a) { return sqrt_n(dot(a, a)); }
DI float clampf(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

// sphere (centre P in the box frame, radius r) against the solid box of half extent hb (cube)
DI void sphere_box(V3 P, float r, float hb, V3& nl, V3& pl, float& gapraw) {
  V3 qv = {clampf(P.x, -hb, hb), clampf(P.y, -hb, hb), clampf(P.z, -hb, hb)};
  V3 d = P - qv;
  float d2 = dot(d, d);
  if (d2 > 1e-12f) {
    float dist = sqrt_n(d2);   // d2 > 1e-12: dist > 1e-6, |d_i| <= dist
    nl = {div_n(d.x, dist), div_n(d.y, dist), div_n(d.z, dist)};
    pl = qv;
    gapraw = dist - r;
  } else {
    float px = hb - fabsf(P.x), py = hb - fabsf(P.y), pz = hb - fabsf(P.z);
    int ax = 0; float best = px;
    if (py < best) { best = py; ax = 1; }
    if (pz < best) { best = pz; ax = 2; }
    float c = ax == 0 ? P.x : (ax == 1 ? P.y : P.z);
    float sgn = c >= 0.f ? 1.f : -1.f;
    nl = {ax == 0 ? sgn : 0.f, ax == 1 ? sgn : 0.f, ax == 2 ? sgn : 0.f};
    pl = {ax == 0 ? sgn * hb : P.x, ax == 1 ? sgn * hb : P.y, ax == 2 ? sgn * hb : P.z};
    gapraw = -best - r;
  }
}

DI float seg_box_dfdt(V3 a, V3 d, float t, float hb) {
  V3 Pt = {a.x + t * d.x, a.y + t * d.y, a.z + t * d.z};
  V3 ex = {Pt.x - clampf(Pt.x, -hb, hb), Pt.y - clampf(Pt.y, -hb, hb), Pt.z - clampf(Pt.z, -hb, hb)};
  return ex.x * d.x + ex.y * d.y + ex.z * d.z;
}

DI Q4 q4p(const float* p) { return {p[0], p[1], p[2], p[3]}; }
DI Q4 qmul(Q4 a, Q4 b) { // xyzw Hamilton product
  return {a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x,
          a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w, a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z};
}
DI Q4 qconj(Q4 a) { return {-a.x, -a.y, -a.z, a.w}; }
DI M3 q2mat(Q4 q) {
  M3 R;
  float x = q.x, y = q.y, z = q.z, w = q.w;
  R.m[0] = 1 - 2 * (y * y + z * z); R.m[1] = 2 * (x * y - z * w); R.m[2] = 2 * (x * z + y * w);
  R.m[3] = 2 * (x * y + z * w); R.m[4] = 1 - 2 * (x * x + z * z); R.m[5] = 2 * (y * z - x * w);
  R.m[6] = 2 * (x * z - y * w); R.m[7] = 2 * (y * z + x * w); R.m[8] = 1 - 2 * (x * x + y * y);
  return R;
}
DI V3 mul(const M3& R, V3 v) {
  return {R.m[0] * v.x + R.m[1] * v.y + R.m[2] * v.z, R.m[3] * v.x + R.m[4] * v.y + R.m[5] * v.z,
          R.m[6] * v.x + R.m[7] * v.y + R.m[8] * v.z};
}
DI V3 mulT(const M3& R, V3 v) {
  return {R.m[0] * v.x + R.m[3] * v.y + R.m[6] * v.z, R.m[1] * v.x + R.m[4] * v.y + R.m[7] * v.z,
          R.m[2] * v.x + R.m[5] * v.y + R.m[8] * v.z};
}
// quat_rotate_inverse(q, v) = v(2w^2-1) - 2w (q_v x v) + 2 q_v (q_v . v)
DI V3 qrot_inv(Q4 q, V3 v) {
  V3 qv = {q.x, q.y, q.z};
  V3 c = cross(qv, v);
  float d = dot(qv, v), s = 2 * q.w * q.w - 1;
  return {v.x * s - 2 * q.w * c.x + 2 * qv.x * d, v.y * s - 2 * q.w * c.y + 2 * qv.y * d,
          v.z * s - 2 * q.w * c.z + 2 * qv.z * d};
}
DI V3 mul(S6 I, V3 v) {
  return {I.xx * v.x + I.xy * v.y + I.xz * v.z, I.xy * v.x + I.yy * v.y + I.yz * v.z,
          I.xz * v.x + I.yz * v.y + I.zz * v.z};
}
DI S6 operator+(S6 a, S6 b) { return {a.xx + b.xx, a.yy + b.yy, a.zz + b.zz, a.xy + b.xy, a.xz + b.xz, a.yz + b.yz}; }
// R * I_local * R^T for a symmetric local inertia
DI S6 rotate_inertia(const M3& R, const float* s /*xx yy zz xy xz yz*/) {
  float Il[9] = {s[0], s[3], s[4], s[3], s[1], s[5], s[4], s[5], s[2]};
  float T[9];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int k = 0; k < 3; k++) T[3 * r + k] = R.m[3 * r] * Il[k] + R.m[3 * r + 1] * Il[3 + k] + R.m[3 * r + 2] * Il[6 + k];
  auto e = [&](int r, int k) { return T[3 * r] * R.m[3 * k] + T[3 * r + 1] * R.m[3 * k + 1] + T[3 * r + 2] * R.m[3 * k + 2]; };
  return {e(0, 0), e(1, 1), e(2, 2), e(0, 1), e(0, 2), e(1, 2)};
}
// R * diag(a, b, c) * R^T: link inertias given in their principal frame (DevParams::inertia_diag: every link of the model) -- 27
// instead of 45 multiply-adds, four times per finger wave and sub-step
DI S6 rotate_inertia_diag(const M3& R, const float* s /*xx yy zz*/) {
  const float a0 = s[0] * R.m[0], a3 = s[0] * R.m[3], a6 = s[0] * R.m[6];
  const float b1 = s[1] * R.m[1], b4 = s[1] * R.m[4], b7 = s[1] * R.m[7];
  const float c2 = s[2] * R.m[2], c5 = s[2] * R.m[5], c8 = s[2] * R.m[8];
  return {a0 * R.m[0] + b1 * R.m[1] + c2 * R.m[2], a3 * R.m[3] + b4 * R.m[4] + c5 * R.m[5], a6 * R.m[6] + b7 * R.m[7] + c8 * R.m[8],
          a0 * R.m[3] + b1 * R.m[4] + c2 * R.m[5], a0 * R.m[6] + b1 * R.m[7] + c2 * R.m[8], a3 * R.m[6] + b4 * R.m[7] + c5 * R.m[8]};
}
// parallel-axis term  m (|d|^2 E - d d^T)
DI S6 pa(float m, V3 d) {
  float dd = dot(d, d);
  return {m * (dd - d.x * d.x), m * (dd - d.y * d.y), m * (dd - d.z * d.z), -m * d.x * d.y, -m * d.x * d.z, -m * d.y * d.z};
}

struct Comp { float m; V3 c; S6 I; };
// a <- a (+) b  (both with positive or zero mass; zero+zero stays at a)
DI void comp_add(Comp& a, const Comp& b) {
  float m = a.m + b.m;
  if (m <= 0.f) return;
  float inv = rcp_n(m);   // m > 0 is a sum of link masses of the model (zero or grams and up): normal
  V3 c = {(a.m * a.c.x + b.m * b.c.x) * inv, (a.m * a.c.y + b.m * b.c.y) * inv, (a.m * a.c.z + b.m * b.c.z) * inv};
  // the two parallel-axis shifts to the common centre of mass are one shift with the reduced mass: m_a |c_a - c|^2 (x) +
  // m_b |c_b - c|^2 (x) = (m_a m_b / m) |c_a - c_b|^2 (x) -- half the instructions, three times per finger and sub-step
  S6 I = a.I + b.I + pa(a.m * b.m * inv, a.c - b.c);
  a.m = m; a.c = c; a.I = I;
}

// in-place inverse of an SPD n x n matrix (row-major full storage) through Cholesky; fully unrolled
template <int n>
DI void spd_inverse(float* A) {
  float L[n * n];
#pragma unroll
  for (int i = 0; i < n; i++)
#pragma unroll
    for (int j = 0; j <= i; j++) {
      float s = A[i * n + j];
#pragma unroll
      for (int k = 0; k < j; k++) s -= L[i * n + k] * L[j * n + k];
      // pivots are clamped: 1e-20 <= s, so 1e-10 <= L_ii and 1 / L_ii <= 1e10.  ASSUMPTION, checked by nothing but the bitwise
      // tests in the regimes they run: an off-diagonal numerator is exactly zero or a cancellation residue of model-scale inertias
      // (a multiple of their ulp, far above 2^-100), so every quotient is zero or normal.  A denormal quotient would round once here
      // and twice in the operator (mantissa product, then ldexp) and could differ in the last bit.  (sqrtf of a clamped
      // value is one v_sqrt_f32 already: the compiler sees the range.  The operator also lets it share the first pivot with
      // spd_solve where a caller branches between the two, as before.)
      if (i == j) L[i * n + i] = opaque(sqrtf(fmaxf(s, 1e-20f)));
      else L[i * n + j] = div_n(s, L[j * n + j]);
    }
  float Li[n * n]; // inverse of L (lower)
#pragma unroll
  for (int c = 0; c < n; c++)
#pragma unroll
    for (int i = c; i < n; i++) {
      float s = (i == c) ? 1.f : 0.f;
#pragma unroll
      for (int k = c; k < i; k++) s -= L[i * n + k] * Li[k * n + c];
      Li[i * n + c] = div_n(s, L[i * n + i]);   // L_ii >= 1e-10 (clamped pivot); s is 1 or a sum of products of quotients of the same kind
    }
#pragma unroll
  for (int i = 0; i < n; i++)
#pragma unroll
    for (int j = 0; j <= i; j++) {
      float s = 0.f;
#pragma unroll
      for (int k = i; k < n; k++) s += Li[k * n + i] * Li[k * n + j];
      A[i * n + j] = s;
      A[j * n + i] = s;
    }
}

// x = A^-1 b for an SPD n x n matrix (row-major, lower triangle read) through Cholesky and two triangular solves; fully
// unrolled.  About 40 % of the arithmetic of spd_inverse + matrix-vector product: the Schur phase of a sub-step without hand
// contacts needs u_B only, not S^-1.
template <int n>
DI void spd_solve(const float* A, const float* b, float* x) {
  float L[n * n], rd[n];   // rd = 1 / L_ii
#pragma unroll
  for (int i = 0; i < n; i++)
#pragma unroll
    for (int j = 0; j <= i; j++) {
      float s = A[i * n + j];
#pragma unroll
      for (int k = 0; k < j; k++) s -= L[i * n + k] * L[j * n + k];
      // (operators: the clamp tells the compiler the range, 1.f / sqrtf is one v_rsq_f32 here)
      if (i == j) { const float d = sqrtf(fmaxf(s, 1e-20f)); L[i * n + i] = d; rd[i] = 1.f / d; }
      else L[i * n + j] = s * rd[j];
    }
  float y[n];
#pragma unroll
  for (int i = 0; i < n; i++) {
    float s = b[i];
#pragma unroll
    for (int k = 0; k < i; k++) s -= L[i * n + k] * y[k];
    y[i] = s * rd[i];
  }
#pragma unroll
  for (int i = n - 1; i >= 0; i--) {
    float s = y[i];
#pragma unroll
    for (int k = i + 1; k < n; k++) s -= L[k * n + i] * x[k];
    x[i] = s * rd[i];
  }
}

DI void tangent_basis(V3 n, V3& t1, V3& t2) {
  V3 e = (fabsf(n.x) < 0.57735f) ? v3(1, 0, 0) : v3(0, 1, 0);
  t1 = cross(e, n);
  float l = norm(t1);
  t1 = {t1.x / l, t1.y / l, t1.z / l};
  t2 = cross(n, t1);
}

// sin and cos of a joint half-angle.  libm's sincosf costs ~145 instructions on gfx950 (its Payne-Hanek large-argument
// reduction is inlined branch-free) and sits 7 times on every wave's critical path per sub-step; joint angles are
// bounded, so one Cody-Waite step to [-pi/4, pi/4] and the classic single-precision minimax kernels (Cephes sinf /
// cosf coefficients, < 1 ulp on the reduced range) do the same job in ~25.  Valid to full accuracy for |h| < ~100.
__device__ __forceinline__ void sincos_joint(float h, float* sn, float* cs) {
  const float kf = rintf(h * 0.6366197723675814f);            // nearest multiple of pi/2
  float r = fmaf(kf, -1.5707963705062866f, h);                 // pi/2 split in two floats (Cody-Waite)
  r = fmaf(kf, 4.371139000186241e-8f, r);
  const float z = r * r;
  const float ps = fmaf(fmaf(fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f), z * r, r);
  const float pc = fmaf(fmaf(fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f), z, 4.166664568298827e-2f), z * z,
                        fmaf(-0.5f, z, 1.0f));
  const int k = (int)kf;
  const bool swap = (k & 1) != 0;
  const float s0 = swap ? pc : ps, c0 = swap ? ps : pc;
  *sn = (k & 2) ? -s0 : s0;
  *cs = ((k + 1) & 2) ? -c0 : c0;
}

// Philox4x32-10 (device-side reset / domain-randomisation stream)
DI void philox4x32(uint32_t out[4], uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  uint32_t c[4] = {c0, c1, c2, c3};
#pragma unroll
  for (int r = 0; r < 10; r++) {
    uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1;
    uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
#pragma unroll
  for (int i = 0; i < 4; i++) out[i] = c[i];
}
DI float u01(uint32_t x) { return (float)(x >> 8) * (1.0f / 16777216.0f); }
