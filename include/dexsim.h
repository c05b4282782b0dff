/*
 * dexsim.h -- C ABI of libdexsim, the MI355X-native vectorised DexHand simulator core.
 *
 * This is the drop-in boundary underneath the reference's Python env surface
 * (reference: dexhand_env/factory.py:93-147 make_env, dexhand_env/tasks/dexhand_base.py:893-942 step,
 * :805-838 reset, :743-803 reset_idx).  The reference has no FFI of its own; every entry
 * point below replaces one *opaque Isaac Gym call site* or one *Python component call* on that path and
 * cites it.  Plain pointers and sizes only: no torch types, no exceptions, int error codes.
 *
 * Memory model: the caller (PyTorch-ROCm host side) allocates device memory and hands pointers in.
 *   - one "arena" of 4-byte words holding every per-env SoA field as [rows][num_envs]
 *     (layout is computed by dexsim_arena_layout and is the *state-buffer contract* that replaces
 *     reference components/physics/tensor_manager.py:139-376);
 *   - a handful of AoS "API tensors" with the reference's own shapes (dof_state (N,26,2), root (N,A,13),
 *     obs_buf (N,O), rew (N), reset (N) u8, episode_step_count (N) i64, ...).
 * The library never allocates or frees per-env memory and never synchronises the stream.
 */
#ifndef DEXSIM_H
#define DEXSIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ fixed topology of the DexHand chain */
#define DEXSIM_NJ        26   /* DOFs: 6 base + 20 finger (reference constants.py:8-11)                 */
#define DEXSIM_NBASE      6
#define DEXSIM_NFINGER    5
#define DEXSIM_NFJ        4   /* joints per finger                                                      */
#define DEXSIM_NACT      18   /* active targets: 6 base + 12 finger controls                            */
#define DEXSIM_NSITE     11   /* right_hand_base, 5 tips, 5 pads (hand_initializer.py:120-134,499-501)  */
#define DEXSIM_NCAP      18   /* collision capsules: 3 palm + 3 per finger                              */
#define DEXSIM_NFSLOT    17   /* net-contact-force slots: 15 finger links, palm, box                    */
#define DEXSIM_FSLOT_PALM 15
#define DEXSIM_FSLOT_BOX  16
#define DEXSIM_KMAX      24   /* max active contacts per env per sub-step (<= 4 box/ground + hand contacts in priority order) */
#define DEXSIM_BISECT_ITERS 10 /* capsule / box narrowphase: bisection steps for the point of the capsule axis nearest to the box
                                (2^-10 of the axis, ~30 um; the gap is stationary there: its error is second order) */
#define DEXSIM_NWKEY 128     /* warm-start cache slots of the contact solver: (capsule * 2 + type) * 2 + sample for hand contacts (< 72),
                                80 + list slot for the (<= 4) box/ground contacts (their tag carries the box corner),
                                88 + (finger joint * 2 + side) for the joint-limit rows (side 0 = lower, 1 = upper) */
/* the warm-start generation of an env advances once per sub-step and once per reset; it wraps at 2^27 so that the cache tags
   8 * generation + corner stay below 2^30 in signed 32-bit arithmetic for any run length (a generation is only ever compared
   with the one before it: a tag can falsely match only if its slot sat unwritten for exactly 2^27 generations) */
#define DEXSIM_WGEN_NEXT(g) (((g) + 1) & 0x07ffffff)
#define DEXSIM_NRESET_SAMPLES 29 /* rand draws of one reset (blind_grasping_task.py:449-547)            */
#define DEXSIM_MAX_OBS_SEG 40

/* task kinds (factory.py:46-62) */
#define DEXSIM_TASK_BASE           0
#define DEXSIM_TASK_BLIND_GRASPING 1

/* control modes (action_processor.py:197-199) */
#define DEXSIM_MODE_POSITION       0
#define DEXSIM_MODE_POSITION_DELTA 1

/* error codes */
#define DEXSIM_OK              0
#define DEXSIM_ERR_ARG         1
#define DEXSIM_ERR_NOT_BOUND   2
#define DEXSIM_ERR_HIP         3
#define DEXSIM_ERR_NO_DEVICE   4
#define DEXSIM_ERR_LAYOUT      5

/* ------------------------------------------------------------------ observation dictionary layout
 * One row block per obs_dict key of the reference (observation_encoder.py:576-758,
 * blind_grasping_task.py:549-653).  obs_all is SoA [DEXSIM_OBS_ALL_DIM][N]; obs_buf (N,O) is the
 * concatenation of the configured policy_observation_keys (observation_encoder.py:783-829). */
#define DEXSIM_OBS_KEYS(X) \
  X(base_dof_pos, 6) X(base_dof_vel, 6) X(active_finger_dof_pos, 12) X(active_finger_dof_vel, 12) \
  X(all_finger_dof_pos, 20) X(all_finger_dof_vel, 20) X(hand_pose, 7) X(hand_pose_arr_aligned, 7) \
  X(contact_forces, 15) X(prev_actions, 18) X(active_prev_targets, 18) X(base_dof_target, 6) \
  X(active_finger_dof_target, 12) X(all_finger_dof_target, 20) X(contact_force_magnitude, 5) \
  X(contact_binary, 5) X(contact_duration, 5) X(fingertip_poses_world, 35) X(fingertip_poses_hand, 35) \
  X(fingerpad_poses_world, 35) X(fingerpad_poses_hand, 35) X(episode_time, 1) X(active_rule_targets, 18) \
  X(object_pos, 3) X(object_vel, 3) X(finger_to_object_distances, 5) X(avg_finger_to_object_distance, 1) \
  X(finger_to_object_height_diff, 5) X(avg_finger_to_object_height_diff, 1) X(hand_to_object_distance, 1) \
  X(fingerpad_distances, 10) X(first_three_fingerpad_centroid, 3) X(thumb_contact, 1) \
  X(other_fingers_contact, 1) X(grasp_state, 1) X(grasp_duration, 1) X(current_stage, 1) \
  X(time_in_stage, 1) X(stage_progress, 1)

enum {
#define X(name, dim) DEXSIM_OBSKEY_##name,
  DEXSIM_OBS_KEYS(X)
#undef X
  DEXSIM_NUM_OBS_KEYS
};
#define DEXSIM_OBS_ALL_DIM 392
#define DEXSIM_OBS_BASE_TASK_DIM 353 /* keys before object_pos exist for every task */

/* ------------------------------------------------------------------ reward terms
 * common: reward_calculator.py:66-221 ; task: blind_grasping_task.py:980-1208 */
#define DEXSIM_REWARD_TERMS(X) \
  X(alive) X(height_safety) X(finger_velocity) X(hand_velocity) X(hand_angular_velocity) X(joint_limit) \
  X(finger_acceleration) X(hand_acceleration) X(hand_angular_acceleration) X(contact_stability) \
  X(s1_height_alignment) X(s1_centroid_positioning) X(s1_object_stability) X(s1_finger_height_consistency) \
  X(s1_thumb_rotation) X(s2_thumb_contact) X(s2_other_fingers_contact) X(s2_grasp_achievement) \
  X(s2_fingerpad_proximity) X(s2_base_stability) X(s3_object_height) X(s3_grasp_maintenance) \
  X(s3_grasp_duration) X(s1_completion) X(s2_completion) X(penetration_penalty)

enum {
#define X(name) DEXSIM_REW_##name,
  DEXSIM_REWARD_TERMS(X)
#undef X
  DEXSIM_NUM_REWARD_TERMS
};
#define DEXSIM_NUM_COMMON_REWARD_TERMS 10
/* reward component rows: [0,26) raw, [26,52) weighted, 52 total, 53..55 termination raw
 * (success, failure_penalty, timeout_penalty), 56..58 termination weighted (step_processor.py:204-219) */
#define DEXSIM_REWROW_WEIGHTED 26
#define DEXSIM_REWROW_TOTAL    52
#define DEXSIM_REWROW_TERM_RAW 53
#define DEXSIM_REWROW_TERM_W   56
#define DEXSIM_NUM_REWROWS     59

/* termination criteria (step_processor.py:133-181, blind_grasping_task.py:1210-1332) */
#define DEXSIM_SUCC_grasp_lift_success 0
#define DEXSIM_NUM_SUCC 1
#define DEXSIM_FAIL_hitting_ground         0
#define DEXSIM_FAIL_box_too_far            1
#define DEXSIM_FAIL_stage1_pregrasp_failed 2
#define DEXSIM_FAIL_stage2_contact_failed  3
#define DEXSIM_FAIL_stage3_grasp_lost      4
#define DEXSIM_NUM_FAIL 5
#define DEXSIM_MASK_SUCCESS 0
#define DEXSIM_MASK_FAILURE 1
#define DEXSIM_MASK_TIMEOUT 2
#define DEXSIM_MASK_SUCC_REASON 3                       /* [NUM_SUCC] */
#define DEXSIM_MASK_FAIL_REASON (3 + DEXSIM_NUM_SUCC)   /* [NUM_FAIL] */
#define DEXSIM_NUM_MASKS (3 + DEXSIM_NUM_SUCC + DEXSIM_NUM_FAIL)

/* global statistics block (device, 64 floats): written once per step by the finalize kernel.
 * termination_manager.py:164-185,259-266 (means / rates), :323-339 (consecutive successes). */
#define DEXSIM_STAT_SUCC_MEAN   0  /* [NUM_SUCC] mean of each success criterion                */
#define DEXSIM_STAT_FAIL_MEAN   4  /* [NUM_FAIL] mean of each failure criterion                */
#define DEXSIM_STAT_SUCCESS_RATE 12
#define DEXSIM_STAT_FAILURE_RATE 13
#define DEXSIM_STAT_TIMEOUT_RATE 14
#define DEXSIM_STAT_CONSECUTIVE_SUCCESSES 15
#define DEXSIM_STAT_NUM_RESETS  16 /* envs reset in this control step                          */
#define DEXSIM_STAT_PHYSICS_STEPS 17 /* physics steps executed in this control step (1 or 2)   */
#define DEXSIM_STAT_MEAN_CONTACTS 18 /* mean active contacts/env in the last sub-step of the step's main physics step */
#define DEXSIM_STAT_MEAN_HAND_CONTACTS 19 /* ... of which hand/box and hand/ground (the rest is box/ground)            */
#define DEXSIM_STAT_USED  20 /* statistics words in use (the rest of the block is reserved)            */
#define DEXSIM_STAT_WORDS 64

/* number of hand bodies published in rigid_body_states: 7 base-chain + 30 finger bodies */
#define DEXSIM_NUM_HAND_BODIES 37

/* ------------------------------------------------------------------ hand model (authored stand-in for the
 * absent MJCF dexhand021_right_simplified_floating.xml, dexhand_base.py:171).
 * Joint j: frame = parent_frame * Trans(poff) * Rot(qoff) * Motion(axis, q); quaternions are xyzw.  Joint 0's parent is the
 * spawn pose.  Finger f (0..4) owns joints 6+4f .. 9+4f, chained; joint 6+4f's parent is joint 5. */
typedef struct DexHandModel {
  float spawn_pos[3];
  float spawn_quat[4];              /* xyzw */
  int   jtype[DEXSIM_NJ];           /* 0 prismatic, 1 revolute */
  float jqoff[DEXSIM_NJ][4];        /* xyzw */
  float jpoff[DEXSIM_NJ][3];
  float jaxis[DEXSIM_NJ][3];        /* unit, in the joint's own frame */
  float mass[DEXSIM_NJ];            /* body carried by joint j; links 0-4 carry none: mass, com and inertia must be 0 there */
  float com[DEXSIM_NJ][3];          /* in joint frame */
  float inertia[DEXSIM_NJ][6];      /* about COM, joint-frame axes: xx yy zz xy xz yz */
  float kp[DEXSIM_NJ], kd[DEXSIM_NJ], armature[DEXSIM_NJ], lo[DEXSIM_NJ], hi[DEXSIM_NJ];
  int   site_parent[DEXSIM_NSITE];  /* joint index the site is welded to */
  float site_q[DEXSIM_NSITE][4];
  float site_p[DEXSIM_NSITE][3];
  int   cap_parent[DEXSIM_NCAP];
  float cap_p0[DEXSIM_NCAP][3];
  float cap_p1[DEXSIM_NCAP][3];
  float cap_r[DEXSIM_NCAP];
  int   cap_fslot[DEXSIM_NCAP];     /* net-contact-force slot of the owning body */
  float hand_friction;
  /* published rigid bodies of the hand actor (rigid_body_states rows): welded to a joint frame
   * (-1 = the fixed spawn frame) by a constant transform */
  int   body_parent[DEXSIM_NUM_HAND_BODIES];
  float body_q[DEXSIM_NUM_HAND_BODIES][4];
  float body_p[DEXSIM_NUM_HAND_BODIES][3];
  int   body_fslot[DEXSIM_NUM_HAND_BODIES]; /* net-contact-force slot or -1 */
} DexHandModel;

/* ------------------------------------------------------------------ resolved configuration
 * (the cfg dict keys the reference consumes, SURVEY.md §8b "cfg keys consumed") */
typedef struct DexSimConfig {
  int   num_envs;
  int   task;                       /* DEXSIM_TASK_* */
  /* sim.* (vec_task.py:226-296, cfg/physics/default.yaml) */
  float dt;
  int   substeps;
  float gravity[3];
  int   num_position_iterations;
  float contact_offset, rest_offset, max_depenetration_velocity;
  float erp;                        /* penetration recovery fraction per sub-step (build's choice) */
  float control_dt;                 /* 2*dt: dexhand_base.py:270-320, physics_manager.py:243-270 */
  int   episode_length;             /* env.episodeLength */
  uint32_t seed;                    /* train.seed */
  /* action (action_processor.py:181-247, 380-434) */
  int   control_mode;
  int   policy_controls_base, policy_controls_fingers;
  int   num_actions;
  float max_deltas[DEXSIM_NACT];
  float active_lower[DEXSIM_NACT], active_upper[DEXSIM_NACT];
  /* observation */
  float contact_binary_threshold;
  int   num_obs;
  int   n_obs_seg;
  int   obs_seg_off[DEXSIM_MAX_OBS_SEG];   /* row offset into obs_all */
  int   obs_seg_len[DEXSIM_MAX_OBS_SEG];
  /* termination (termination_manager.py:26-75) */
  int   height_safety_enabled;
  float handbase_threshold, fingertip_threshold;
  int   active_success_mask;        /* bit i = success criterion i active */
  int   active_failure_mask;
  float success_reward, failure_penalty, timeout_penalty;
  int   max_consecutive_successes;
  /* reward weights (reward_weights section of the task YAML) */
  float reward_weight[DEXSIM_NUM_REWARD_TERMS];
  /* ground + box (dexhand_base.py:632-638, blind_grasping_task.py:138-144) */
  float ground_friction;
  int   has_box;
  float box_size, box_mass, box_friction, box_xy_range, box_z;
  /* BlindGrasping task params (blind_grasping_task.py:146-199) */
  float height_threshold, contact_duration_threshold_s;
  int   contact_duration_threshold_steps;  /* int(threshold / control_dt), :271-273 */
  int   min_fingers_for_grasp;
  float max_box_distance, stage1_duration, stage2_duration;
  float hand_translation_range, hand_rotation_range, thumb_rotation_range, other_finger_range;
  float stage2_contact_success_threshold;
  float height_alignment_decay, centroid_positioning_decay, object_stability_decay;
  float first_three_height_consistency_decay, fingerpad_proximity_decay, base_stability_decay;
  float geometric_penetration_factor, proximity_min_distance_factor, penetration_depth_scale;
  float height_tolerance, centroid_tolerance, position_drift_tolerance, velocity_tolerance;
  /* per-env domain randomisation of the box (BASELINE config #5; new capability).  With dr_enabled every env draws its mass from
   * [dr_mass_lo, dr_mass_hi] and its friction from [dr_mu_lo, dr_mu_hi] once, at create; dexsim_create refuses (DEXSIM_ERR_ARG)
   * dr_mass_lo <= 0, dr_mu_lo < 0, lo > hi and non-finite bounds. */
  int   dr_enabled;
  float dr_mass_lo, dr_mass_hi, dr_mu_lo, dr_mu_hi;
  uint32_t dr_seed;
  /* static box actor (the harness's contact-test box, examples/dexhand_test.py:950-1024: gym.create_box with
   * fix_base_link = True at a fixed pose, identity orientation).  With box_fixed the box never moves: no gravity, no
   * box/ground contacts, infinite mass in the hand/box contact rows; resets leave it where it is.  Works with either task
   * (BaseTask has no box of its own: has_box = 1 then adds the second actor). */
  int   box_fixed;
  float box_fixed_pos[3];
  /* Joint limits as unilateral solver rows (round 3; the reference's limits are PhysX articulation limits, dof_props lower / upper,
   * tensor_manager.py:547-554).  With joint_limit_rows != 0 every finger joint within joint_limit_margin (rad) of a limit gets a
   * one-row speculative constraint (J = +-e_j, gap = distance to the limit, no friction) in the contact solver -- for the fingers
   * that have at least one contact in the sub-step: without contact forces the PD drive cannot push a joint across a limit its
   * own target respects, and the position clamp behind the integration stays as the safety net in every case.  List order: a
   * finger's limit rows follow that finger's contacts; they count against DEXSIM_KMAX; each is a solver block of its own. */
  int   joint_limit_rows;
  float joint_limit_margin;
} DexSimConfig;

/* ------------------------------------------------------------------ arena layout */
typedef struct DexSimField {
  char   name[40];
  int    rows;       /* field occupies rows*num_envs words at offset */
  int    is_int;     /* 1: int32 words, 0: float32 */
  size_t offset;     /* in 4-byte words from arena base */
} DexSimField;

/* API tensors (AoS, reference shapes).  All device pointers; any may be NULL except obs_buf/rew/reset. */
typedef struct DexSimBuffers {
  void*    arena;              /* arena_words * 4 bytes                                             */
  float*   stats;              /* DEXSIM_STAT_WORDS floats                                          */
  int*     counters;           /* DEXSIM_STAT_WORDS ints, scratch for the statistics reduction      */
  float*   obs_buf;            /* (N, num_obs) row-major  -- DexHandBase.obs_buf                    */
  float*   rew_buf;            /* (N,)                                                              */
  uint8_t* reset_buf;          /* (N,) bool                                                         */
  int64_t* episode_step_count; /* (N,) int64 (initialization_manager.py:47-49)                      */
  int64_t* episode_length;     /* (N,) int64 extras["episode_length"] (step_processor.py:221-232)   */
  float*   dof_state;          /* (N, 26, 2)  gym.refresh_dof_state_tensor                          */
  float*   root_state;         /* (N, A, 13)  gym.refresh_actor_root_state_tensor; A = 1 + has_box  */
  float*   rigid_body_states;  /* (N, B, 13)  filled by dexsim_refresh_body_states only             */
  float*   contact_forces_all; /* (N, B, 3)   filled by dexsim_refresh_body_states only             */
  float*   full_dof_targets;   /* (N, 26)     ActionProcessor.full_dof_targets                      */
  float*   reset_samples;      /* (N, 29) uniforms in [0,1) or NULL -> device Philox stream         */
  uint8_t* masks;              /* (DEXSIM_NUM_MASKS, N) bool rows, extras masks (step_processor.py:221-232,
                                  termination_manager.py:246-256): success, failure, timeout,
                                  success_reason[NUM_SUCC], failure_reason[NUM_FAIL]; may be NULL     */
  float*   raw_targets;        /* (N, 18) or NULL: output of a host-side custom action rule
                                  (ActionRules.set_action_rule, rules.py:211-224) replacing the built-in
                                  position / position_delta rule; filters + coupling still run in-kernel */
} DexSimBuffers;

typedef struct DexSim* dexsim_t;

/* sizeof() of {DexHandModel, DexSimConfig, DexSimField, DexSimBuffers}: lets a foreign-language
 * binding verify its struct mirrors before passing pointers. */
int dexsim_struct_sizes(size_t out[4]);

/* Layout of the arena for this configuration.  Replaces TensorManager.acquire_tensor_handles
 * (tensor_manager.py:80-136): tells the host what to allocate and where each field lives. */
int dexsim_arena_layout(const DexSimConfig* cfg, DexSimField* fields, int max_fields, int* n_fields,
                        size_t* arena_words);

/* obs_dict key table: name / row offset / dim of key i (0 <= i < DEXSIM_NUM_OBS_KEYS). */
int dexsim_obs_key_info(int i, const char** name, int* offset, int* dim);
/* reward term name i (0 <= i < DEXSIM_NUM_REWARD_TERMS). */
int dexsim_reward_term_name(int i, const char** name);
/* rigid body name i of the hand actor (0 <= i < DEXSIM_NUM_HAND_BODIES). */
int dexsim_body_name(int i, const char** name);

/* create_sim + load_asset + create_actor for every env (vec_task.py:298-311,
 * hand_initializer.py:209-257,365-422, blind_grasping_task.py:300-366). No per-env allocation. */
int dexsim_create(const DexSimConfig* cfg, const DexHandModel* model, int device, dexsim_t* out);
int dexsim_destroy(dexsim_t h);

/* gym.acquire_*_tensor + gymtorch.wrap_tensor + gym.prepare_sim (tensor_manager.py:99-136,
 * dexhand_base.py:431): bind caller-owned device memory. */
int dexsim_bind(dexsim_t h, const DexSimBuffers* bufs);

/* Zero all state, put the hand at the spawn pose, box at its default pose, FSM at stage 1, draw the
 * per-env DR parameters.  (scene construction, dexhand_base.py:609-672.) */
int dexsim_init_state(dexsim_t h, void* stream);

/* ActionProcessor.process_actions + gym.set_dof_position_target_tensor
 * (action_processor.py:284-352); also ObservationEncoder.update_prev_actions (:287-296).
 * actions: (N, num_actions) device.  zero_targets != 0 reproduces the pre-finalize_setup branch
 * (:305-318). */
int dexsim_process_actions(dexsim_t h, const float* actions, int zero_targets, void* stream);

/* Opens a control step whose action stage ran on the host (custom post-action filters / coupling rule,
 * action_processor.py:698-720, write targets and active_prev_targets into the arena directly): what
 * dexsim_process_actions does for the device-side step bookkeeping (new stamp of the device-side reset gate, contact
 * statistics words), without touching targets. */
int dexsim_begin_step(dexsim_t h, void* stream);

/* PhysicsManager.step_physics = gym.simulate + fetch_results + 4 refreshes
 * (physics_manager.py:73-119): one sim.dt = `substeps` sub-steps for every env, then publish
 * dof_state/root_state and the compact L1 state.  gate_on_reset != 0 makes every kernel a no-op unless
 * the device-side "some env reset this step" flag is set (reset_manager.py:180 without a host sync). */
int dexsim_physics_step(dexsim_t h, int gate_on_reset, void* stream);

/* StepProcessor.process_physics_step (step_processor.py:37-131) up to and including the reset of
 * finished envs and the extra physics step.  obs_only != 0 = compute_observations +
 * concatenate_observations only (dexhand_base.py:811-834). */
int dexsim_post_physics(dexsim_t h, int obs_only, void* stream);

/* DexHandBase.step (dexhand_base.py:893-942): process_actions, physics, post-physics, in-step resets,
 * conditional extra physics step, extras statistics.  No host synchronisation.  Two halves of substeps / 4 + substeps % 4
 * launches each (with substeps == 4: two launches): the ungated half carries the whole control step up to the reset gate
 * (actions on its first launch, post-physics on its last), its device-gated twin the extra physics step, with reset
 * phase 1 and the statistics on its last launch.  Same results as the three staged calls above. */
int dexsim_step(dexsim_t h, const float* actions, void* stream);

/* DexHandBase.reset_idx (dexhand_base.py:743-803) for caller-chosen envs: env_ids is a device array
 * of k int64.  Includes the unconditional physics step of ResetManager.reset_idx (reset_manager.py:180). */
int dexsim_reset_idx(dexsim_t h, const int64_t* env_ids, int k, void* stream);

/* DexHandBase.reset (dexhand_base.py:805-838): reset_idx(all) + observations + post_physics_step. */
int dexsim_reset(dexsim_t h, void* stream);

/* gym.refresh_rigid_body_state_tensor + refresh_net_contact_force_tensor for the full (N,B,*)
 * tensors (physics_manager.py:108-109), materialised on demand. */
int dexsim_refresh_body_states(dexsim_t h, void* stream);

/* gym.set_dof_state_tensor_indexed / set_actor_root_state_tensor_indexed
 * (physics_manager.py:146-151, reset_manager.py:153-158): ingest the AoS API tensors for k envs.
 * (The contact solver's warm-start cache -- arena field `wlam`, generation `wgen` -- is invalidated by resets, not by these
 * setters: after a teleport a stale entry is only the starting guess of the first sub-step's solve.) */
int dexsim_set_dof_state_indexed(dexsim_t h, const int64_t* env_ids, int k, void* stream);
int dexsim_set_root_state_indexed(dexsim_t h, const int64_t* env_ids, int k, void* stream);

/* Rollout sink (new capability, SURVEY.md 8e / 8f-1: the "PPO buffer" end of the path): besides obs_buf / rew_buf /
 * reset_buf the post-physics flush of every following dexsim_step / dexsim_post_physics also writes the step's
 * observations (N, num_obs) f32, rewards (N) f32 and done flags (N) u8 to these device pointers -- typically row t of
 * the caller's (T, N, ...) rollout tensors -- so that collecting a rollout needs no copy kernels.  Any pointer may be
 * NULL; all NULL switches the sink off.  The pointers are kernel arguments: no device memory is touched by this call. */
int dexsim_set_step_sink(dexsim_t h, float* obs, float* rew, uint8_t* done);

/* Statistics sink: the launch that closes a control step (finalize_stats: the cross-env means / rates of
 * TerminationManager.evaluate, termination_manager.py:160-185, and consecutive successes, :323-339) also copies the first
 * DEXSIM_STAT_USED words of the statistics block to `dst` -- row t of the caller's (T, DEXSIM_STAT_WORDS) rollout tensor -- so that
 * envs sharded over ranks can reduce their whole-population statistics with ONE small all-reduce per rollout (rollout.py:
 * reduce_stats) instead of one per step.  NULL switches it off.  Kernel argument like the step sink. */
int dexsim_set_stats_sink(dexsim_t h, float* dst);

/* get_observations_dict() (dexhand_base.py:948-956) is served from the arena field obs_all: 392 SoA rows per env that the post
 * block writes in every step (mode 0, the default: every key of the reference's obs_dict is a view).  A training loop reads
 * obs_buf only -- the configured policy keys -- so mode 1 ("policy") stops materialising the rows: 1 568 B per env and step less
 * to write; the host side then serves the policy keys as views of obs_buf and raises on any other key.  Kernel argument. */
int dexsim_set_obs_dict_mode(dexsim_t h, int mode);

/* Phase probe (measurement, SURVEY.md 8d: the contact-solve sub-metric on the PRODUCTION kernel): with `buf` set --
 * 4 x ceil(num_envs / 64) uint32 on the device, zeroed by the caller -- every following physics launch adds, per workgroup,
 * shader-clock ticks (s_memtime) to buf[4 w + 0] = phases 3 + 4 of the general contact path (contact rows +
 * the block solver's sweeps), [4 w + 1] = the whole launch (ungated launches), [4 w + 3] = phase 4 alone, and counts in
 * [4 w + 2] the sub-steps that ran the general path.  Solver time = launch time (HIP events) x buf[0] / buf[1].  NULL switches it
 * off (the default; the probe then costs two scalar branches per sub-step). */
int dexsim_set_phase_probe(dexsim_t h, uint32_t* buf);

/* DexHandBase.pre_physics_step keeps `self.actions = actions.clone()` (dexhand_base.py:851).  With a destination set here
 * ((N, num_actions) f32 on the device, or NULL to switch off) the action block writes that copy itself, so the host side
 * needs no clone kernel per step.  Kernel argument like the step sink. */
int dexsim_set_action_copy(dexsim_t h, float* dst);

/* Test / profiling hooks: run one pipeline stage on the bound buffers. */
#define DEXSIM_STAGE_DYNAMICS 0  /* FK + CRBA + bias + factorisation + narrowphase + row build (stand-alone kernel) */
#define DEXSIM_STAGE_SOLVE    1  /* PGS contact-impulse solve + integrate (stand-alone kernel)      */
#define DEXSIM_STAGE_PUBLISH  2  /* FK of sites, AoS dof_state/root publication                     */
#define DEXSIM_STAGE_POST     3  /* fused obs + FSM + termination + reward                          */
#define DEXSIM_STAGE_RESET    4  /* masked reset of envs whose reset_buf is set                     */
#define DEXSIM_STAGE_FINALIZE 5  /* statistics                                                      */
#define DEXSIM_STAGE_SUBSTEP  6  /* one sub-step (DYNAMICS + SOLVE + integration + publication, contact statistics) as its own launch */
#define DEXSIM_STAGE_PHYSICS  7  /* physics step alone: all `substeps` of a sim.dt (substeps / 4 + substeps % 4 launches) */
#define DEXSIM_STAGE_STEP     8  /* the ungated half of dexsim_step: actions + all sub-steps + post-physics (re-uses  */
                                 /* the action pointer of the last dexsim_step; advances the simulation)                */
int dexsim_run_stage(dexsim_t h, int stage, void* stream);

/* Time `launches` launches of one stage, each bracketed by a hipEvent pair and a host synchronisation, and return the
 * mean duration in microseconds.  The event fences make every launch start from a cold L2, so these are upper bounds
 * (bench.py uses them for the stand-alone kernels only). */
int dexsim_time_stage(dexsim_t h, int stage, int launches, void* stream, float* mean_us);

/* In-situ timing of the ungated half of dexsim_step (the launches that carry the actions, the sub-steps and the
 * post-physics block; one launch when substeps == 4): enable != 0 starts recording a hipEvent pair around it on every
 * following dexsim_step (ring of 64, no host synchronisation, so the launches stay back to back as in production); enable == 0 stops,
 * synchronises and returns the mean duration in microseconds over the *n recorded steps.  (The event fences still
 * cost the kernel its warm L2: +30 % on MI355X; bench.py therefore times the whole region instead.) */
int dexsim_step_timing(dexsim_t h, int enable, float* mean_us, int* n);

/* ------------------------------------------------------------------ save, restore and fork of simulation state
 * (new capability: the reference keeps its state inside PhysX and a dozen Python objects and cannot hand it out)
 *
 * The STATE RECORD of one env is everything that decides how that env continues:
 *   - its share of every *persistent* arena field (DEXSIM_STATE_FIELDS in dexsim_device.h: every arena field except the
 *     hand-off scratch of a single sub-step -- joint frames, factors, manifold, contact rows).  That includes the warm-start
 *     cache (wlam, wgen), FSM stage and timers, contact durations, previous-velocity rows, episode counters, reward
 *     bookkeeping, the per-env box parameters (box_mass, box_mu) and reset_count, the Philox key of the env's next reset;
 *   - its rows of the published API tensors: obs_buf, rew_buf, reset_buf, episode_step_count, episode_length, dof_state,
 *     root_state, full_dof_targets and its column of masks.  They are stored and restored, not recomputed: a load launches
 *     no publication and changes no bit of any env outside its id list.  rigid_body_states / contact_forces_all are
 *     materialised on access (dexsim_refresh_body_states) and are not part of the record.
 * A record is defined at control-step boundaries (between two dexsim_step calls, after dexsim_reset / dexsim_reset_idx), and at
 * sub-step boundaries for the staged entry points (dexsim_physics_step, DEXSIM_STAGE_SUBSTEP).  The hand-off between the
 * stand-alone DEXSIM_STAGE_DYNAMICS and DEXSIM_STAGE_SOLVE launches is deliberately not part of it.
 *
 * Records live in a caller-allocated device buffer, the STATE BANK, of `capacity` slots:
 * record_words * pad64(capacity) * 4 bytes (pad64 = rounded up to a multiple of 64), 16-byte aligned.  Its internal layout is
 * the library's (slot-fastest SoA; dexsim_state_layout describes one record) and is versioned by DEXSIM_STATE_VERSION: keep the
 * version, record_words and the configuration next to any bank that outlives the process.  The library allocates nothing.
 *
 * Outside the records there are two small caller-owned global blocks, `stats` and `counters` (DexSimBuffers; the latter holds
 * the consecutive-successes count and the reward calculator's lazy-init flag), and ONE host-side word, the step stamp.  A full
 * snapshot of an instance = a bank of >= NS slots saved in identity mode + copies of stats and counters + the stamp.
 *
 * Semantics:
 *   - Whole-instance restore is bitwise: a snapshot loaded into the same instance, or into a fresh one with the same
 *     configuration and model, continues bit for bit.
 *   - A fork or indexed load onto arbitrary lanes is exact for the moved envs at that moment but need not continue bitwise
 *     like the source: the 64 envs of a workgroup take workgroup-uniform decisions together (hand-clear or general contact
 *     path, the wave-wide stop of the box sweeps).  A whole workgroup copied onto another in the same lane order does.
 *   - Resets key Philox by (env index, reset_count): a forked env draws its own randoms at its next reset unless
 *     reset_samples are injected.
 *   - box_mass / box_mu travel with the record: a fork takes the source's box. */
#define DEXSIM_STATE_VERSION 1

/* Layout of one state record for this configuration: name, rows (= words), is_int and the word offset inside the record of
 * every section, in record order; the arena sections carry the arena field's name, the API sections "api.<tensor>"
 * (64-bit tensors as two int32 words lo/hi per element, reset_buf as one word, the mask column packed four bytes per word).
 * Slot s of a bank keeps word w of a section at bank[(offset + w) * pad64(capacity) + s]; the one quad-layout section,
 * wlam, keeps word 4 q + c at bank[offset * pad64(capacity) + (q * pad64(capacity) + s) * 4 + c], like the arena.
 * Needs no device.  DEXSIM_ERR_LAYOUT when the table is too small (fields == NULL just counts). */
int dexsim_state_layout(const DexSimConfig* cfg, DexSimField* fields, int max_fields, int* n_fields, size_t* record_words);

/* Save the records of k envs into bank slots / load them back.  env_ids and slots are device arrays of k int64, ids in
 * [0, num_envs), slots in [0, capacity); a lane whose id or slot is out of range moves nothing.  For a load, env_ids must
 * not repeat.  env_ids == NULL together with slots == NULL is the identity over ALL NS = pad64(num_envs) lanes (k is
 * not used but must not be negative): the arena records of the padded lanes are included, because they take part in their workgroup's decisions; it
 * needs capacity >= NS.  Stream-ordered, no synchronisation, no allocation. */
int dexsim_save_state(dexsim_t h, const int64_t* env_ids, const int64_t* slots, int k, void* bank, int64_t capacity, void* stream);
int dexsim_load_state(dexsim_t h, const int64_t* env_ids, const int64_t* slots, int k, const void* bank, int64_t capacity, void* stream);

/* Fork inside one instance: record of env src_ids[i] -> env dst_ids[i], i < k (device arrays of int64 in [0, num_envs)).
 * A source may repeat.  PRECONDITION (not checked here): the destinations are unique and none of them is also a source. */
int dexsim_copy_envs(dexsim_t h, const int64_t* src_ids, const int64_t* dst_ids, int k, void* stream);

/* The step stamp: the only host-side simulation state.  Its parity selects the contact-statistics words of the counters
 * block and its value is the device-side reset gate.  Host-only calls: no launch, no synchronisation.  Valid stamps are
 * [1, 0x3ffffffe]. */
int dexsim_get_step_stamp(dexsim_t h, int* stamp);
int dexsim_set_step_stamp(dexsim_t h, int stamp);

/* ------------------------------------------------------------------ camera sensors: depth, segmentation and colour images
 * Replaces the reference's graphics layer for sensors: GraphicsManager.create_camera / set_camera_location /
 * render_all_cameras / capture_frame (graphics_manager.py:56-179) and the fixed "video camera" of VideoManager
 * (video_manager.py:56-147: 75 deg horizontal FOV, behind env 0, looking at the hand).  No encoder, viewer or stream: a recorder
 * is a caller-side loop over frames.
 *
 * Everything the engine collides is analytic -- DEXSIM_NCAP capsules welded to joint frames, one cube, the ground plane z = 0 --
 * so a camera is an exact ray-caster over those primitives.  Rendering is a pure function of the persistent state (arena fields q,
 * box_pos, box_quat): it changes no arena word, no API tensor, no statistics or counters word and not the step stamp.
 *
 * PIXEL MODEL.  Pinhole camera.  Pixel (x, y), x to the right, y downwards, row-major; its ray leaves the eye through the pixel
 * centre: d = normalize(forward + sx right + sy up), sx = (2 (x + 0.5) / W - 1) tan(hfov / 2),
 * sy = (1 - 2 (y + 0.5) / H) tan(hfov / 2) H / W (the vertical extent follows from the aspect ratio).
 * Every primitive contributes the point where the ray ENTERS it (a camera inside a primitive does not see it; the ground is hit from
 * either side); a hit's depth is its distance along the optical axis, t (d . forward).  Hits with depth outside
 * [near_clip, far_clip] are dropped; the nearest remaining hit wins.
 *   depth  f32: that depth, or +inf without a hit
 *   seg    i32: DEXSIM_SEG_NONE without a hit, DEXSIM_SEG_GROUND, DEXSIM_SEG_BOX, DEXSIM_SEG_CAPSULE0 + c for capsule c in
 *          DexHandModel order (cap_fslot maps a capsule to its finger link or the palm)
 *   rgba   4 x u8: alpha 255; channel = round(palette[p][channel] * (ambient + (1 - ambient) * max(0, n . l))), n the outward
 *          surface normal at the hit, l the unit vector towards the one directional light; palette entry p: 0 ground, 1 box, 2 palm,
 *          3 + f finger f (= cap_fslot / 3).  No hit: the background colour.  No shadows, no textures. */
#define DEXSIM_SEG_NONE     0
#define DEXSIM_SEG_GROUND   1
#define DEXSIM_SEG_BOX      2
#define DEXSIM_SEG_CAPSULE0 3
#define DEXSIM_RENDER_AMBIENT 0.35f
#define DEXSIM_RENDER_LIGHT { 2.0f / 7.0f, 3.0f / 7.0f, 6.0f / 7.0f }   /* unit vector towards the light, world frame */
#define DEXSIM_RENDER_NPALETTE 8
#define DEXSIM_RENDER_PALETTE { {150, 150, 140}, {215, 150, 60}, {200, 200, 210}, {230, 80, 70}, {80, 180, 90}, \
                                {70, 120, 230}, {220, 200, 70}, {180, 90, 200} }   /* 8-bit R, G, B */
#define DEXSIM_RENDER_BACKGROUND { 135, 170, 215 }
#define DEXSIM_RENDER_MAX_DIM 4096

/* A camera.  The look-at pair is given in the PARENT frame: parent_joint = -1 is the env's world frame, 0 .. DEXSIM_NJ - 1 mounts
 * the camera on that joint's frame (5 = the palm joint: an eye-in-hand camera).  Up is the parent's +z axis; when the sine of the
 * angle between the view direction and that axis is below 1e-6 the parent's +y axis takes its place (and a zero-length view
 * direction becomes the parent's +x), so the resolved frame never holds a NaN. */
typedef struct DexSimCamera {
  int   width, height;           /* [1, DEXSIM_RENDER_MAX_DIM] */
  float hfov_deg;                /* horizontal field of view, (0, 180); the reference's video camera uses 75 */
  float near_clip, far_clip;     /* metres along the optical axis, near_clip < far_clip */
  int   parent_joint;
  float eye[3], target[3];       /* shared by all rendered envs unless dexsim_render gets per-env arrays */
} DexSimCamera;

/* sizeof(DexSimCamera), for bindings to verify their mirror (dexsim_struct_sizes keeps its four entries). */
int dexsim_camera_struct_size(size_t* out);

/* The SCENE RECORD of one rendered env is the world-space geometry the ray kernel consumes: DEXSIM_SCENE_WORDS 4-byte words, one
 * contiguous record per rendered env (AoS: all pixels of an image share one record and fetch it through the scalar cache).
 * Sections, in record order (dexsim_render_layout reports name, words, is_int and word offset of each):
 *   cam_eye 3, cam_right 3, cam_up 3, cam_forward 3   the resolved camera: eye and the orthonormal frame, world coordinates
 *   box_center 3, box_rot 9, box_half 1               rotation row-major, world <- box; box_half = half edge, 0 = "no box"
 *   box_eye 3, box_light 3                            eye relative to the centre and the light direction, in box coordinates
 *   cap_rgb DEXSIM_NCAP (int)                         palette colour of each capsule, R | G << 8 | B << 16
 *   reserved 3
 *   capsules DEXSIM_NCAP x DEXSIM_RCAP_WORDS          per capsule, word offsets DEXSIM_RCAP_*: endpoints a, b, radius, and what
 *                                                     is the same for every ray of the image (u = unit axis, o = eye - a) */
#define DEXSIM_RCAP_A      0   /* [3] endpoint a (cap_p0), world                 */
#define DEXSIM_RCAP_R      3   /* radius                                         */
#define DEXSIM_RCAP_B      4   /* [3] endpoint b (cap_p1), world                 */
#define DEXSIM_RCAP_LEN    7   /* |b - a|                                        */
#define DEXSIM_RCAP_U      8   /* [3] u = (b - a) / |b - a|                      */
#define DEXSIM_RCAP_UO    11   /* u . o                                          */
#define DEXSIM_RCAP_O     12   /* [3] o = eye - a                                */
#define DEXSIM_RCAP_INVR  15   /* 1 / radius                                     */
#define DEXSIM_RCAP_N     16   /* [3] u x o                                      */
#define DEXSIM_RCAP_CA    19   /* |eye - a|^2 - r^2                              */
#define DEXSIM_RCAP_CB    20   /* |eye - b|^2 - r^2                              */
#define DEXSIM_RCAP_LO    21   /* light . o                                      */
#define DEXSIM_RCAP_LU    22   /* light . u                                      */
#define DEXSIM_RCAP_R2    23   /* r^2                                            */
#define DEXSIM_RCAP_WORDS 24
#define DEXSIM_SCENE_WORDS (52 + DEXSIM_NCAP * DEXSIM_RCAP_WORDS)

/* Layout of one scene record (DexSimField convention: rows = words of the section, offset in words inside the record).  Needs no
 * device.  DEXSIM_ERR_LAYOUT when the table is too small (fields == NULL just counts). */
int dexsim_render_layout(DexSimField* fields, int max_fields, int* n_fields, size_t* scene_words);

/* Render camera `cam` for k envs: GraphicsManager.render_all_cameras + capture_frame (graphics_manager.py:56-179).
 *   eye, target  optional device (k, 3) f32 arrays overriding cam->eye / cam->target per rendered env (per-env placement,
 *                camera randomisation); NULL = the shared pair
 *   env_ids      device array of k int64; NULL = all num_envs envs in order (k is then not used), as in dexsim_save_state.  A lane
 *                whose id is outside [0, num_envs) renders nothing: its record and its images are left as they are
 *   scene        caller workspace of k x DEXSIM_SCENE_WORDS floats, 16-byte aligned; it holds the scene records afterwards
 *   depth (k, H, W) f32, rgba (k, H, W, 4) u8 (4-byte aligned), seg (k, H, W) i32: any may be NULL, not all three
 * Two launches (scene records: one lane per env; rays: one lane per pixel), stream-ordered, no allocation, no synchronisation.
 * DEXSIM_ERR_ARG for a NULL or unbound handle, width or height outside [1, DEXSIM_RENDER_MAX_DIM], k * width * height >= 2^31,
 * hfov_deg outside (0, 180), near_clip >= far_clip, parent_joint outside [-1, DEXSIM_NJ), k < 0, a NULL scene or no output. */
int dexsim_render(dexsim_t h, const DexSimCamera* cam, const float* eye, const float* target, const int64_t* env_ids, int k,
                  float* scene, float* depth, uint8_t* rgba, int32_t* seg, void* stream);

/* ------------------------------------------------------------------ range sensors: batched ray casts with distance, hit and normal
 * A few dozen arbitrary rays, each mounted on a joint frame of the hand or on the env's world frame, cast against the ground, the box
 * and the hand's capsules by the intersection rule of the camera sensors above: the entry point, DEXSIM_RAY_MAX and
 * DEXSIM_RAY_SKIP_PARENT are declared and documented in dexsim_ray.h, which is part of this header. */
#include "dexsim_ray.h"

/* ------------------------------------------------------------------ body Jacobians, mass matrix and gravity force
 * The counterparts of gym.acquire_jacobian_tensor / refresh_jacobian_tensors and gym.acquire_mass_matrix_tensor /
 * refresh_mass_matrix_tensors for the hand actor, for Cartesian fingertip control and inverse kinematics, operational-space and
 * impedance control, gravity compensation and grasp analysis (J^T maps contact forces to joint torques).  Everything here is a
 * pure function of q: no velocity-product terms.  Both calls are stream-ordered, never synchronise and allocate nothing, and
 * neither writes any arena word, API tensor, statistics word, counter or the step stamp.
 *
 * ROWS.  Output row i describes env env_ids[i] (device array of k int64).  env_ids == NULL: row i is env i, and k must be
 * num_envs.  A row whose id is outside [0, num_envs) is skipped: its output row is left untouched, as the camera call leaves
 * the images of such a row.
 * Q OVERRIDE.  q == NULL: the envs' current q (arena).  q != NULL: a device (k, 26) row-major array of joint positions in
 * dof_state order that takes the place of the state; env_ids is then ignored and k may be any positive number (the model is
 * shared by all envs: a batched kinematics service for planners and IK loops).  A row of q equal to an env's current q gives
 * that env's output bit for bit.
 *
 * JACOBIAN  jac (k, nb, 6, 26) f32 row-major, 16-byte aligned.  bodies: HOST array of nb hand-body indices in
 * [0, DEXSIM_NUM_HAND_BODIES), in the row order of rigid_body_states and the name order of the body-name table; NULL = all
 * DEXSIM_NUM_HAND_BODIES in order (nb must then be DEXSIM_NUM_HAND_BODIES).  Rows 0-2: world linear velocity of the body-frame
 * origin (the point rigid_body_states publishes in columns 0:3, whose velocity it publishes in 7:10); rows 3-5: world angular
 * velocity; column j: DOF j in dof_state order.  Contract: jac[i, b] @ qd == rigid_body_states[env, b, 7:13].  Columns of
 * joints that do not move the body are written as exact 0.0f (the buffer need not be zeroed); body 0 (hand_mount, welded to
 * the fixed spawn frame) is all zeros.  The bodies ride on the joint frames rigid_body_states places them on; a model whose
 * body_parent says otherwise is refused.
 *
 * MASS MATRIX  mass (k, 26, 26) f32, 16-byte aligned: the joint-space inertia M(q) of the articulated hand (composite-rigid-body
 * method), general link inertias.  No armature and no PD terms: the integrator's M^ adds diag(armature + h (kd + h kp)) to it.
 * Both triangles are written from one computed value (M == M^T bitwise); the finger-finger cross blocks are exact zeros.
 * GRAVITY FORCE  gravity (k, 26) f32: dV/dq for cfg.gravity, i.e. the bias force of the recursive Newton-Euler pass at qd = 0 --
 * the generalized force a controller ADDS to hold the hand (default model, gravity (0, 0, -9.81): entry 2, the z slide, is about
 * +5.17 N).  Either of mass and gravity may be NULL, not both.
 *
 * DEXSIM_ERR_ARG (with a dexsim_last_error text; no device needed): NULL handle, k <= 0, env_ids == NULL without q and
 * k != num_envs, nb outside [1, DEXSIM_NUM_HAND_BODIES], a body index out of range, bodies == NULL with
 * nb != DEXSIM_NUM_HAND_BODIES, a NULL or misaligned output.  DEXSIM_ERR_NOT_BOUND before dexsim_bind. */
int dexsim_body_jacobian(dexsim_t h, const int64_t* env_ids, int k, const float* q, const int* bodies, int nb, float* jac,
                         void* stream);
int dexsim_mass_matrix(dexsim_t h, const int64_t* env_ids, int k, const float* q, float* mass, float* gravity, void* stream);

/* ------------------------------------------------------------------ fingertip inverse kinematics in control space
 * Batched damped-least-squares IK for the five fingertip (or fingerpad) POSITIONS, solved for the 18 active targets of the action
 * stage (the controls of DexSimConfig::active_lower / active_upper, coupled to the 26 DOFs as the action stage couples them), every
 * iteration inside one launch.  The call is stream-ordered, never synchronises and allocates nothing, and writes no arena word,
 * API tensor, statistics word, counter or the step stamp.  ROWS and the q0 OVERRIDE are those of dexsim_body_jacobian: row i is env
 * env_ids[i] (NULL: env i, k == num_envs) and starts from its current q; with q0 != NULL, a device (k, 26) array, row i starts
 * from q0[i] and env_ids is ignored.  A row whose id is outside [0, num_envs) leaves its output rows untouched.
 *
 * THE ITERATION.  q(u): DOF d = sum over the controls of scale * u_c (thumb DIP, finger DIPs: two DOFs per control; control 9
 * spreads index, ring and, twice as far, pinky); DOF 14, driven by no control, is 0.  Start: u0_c = clamp(q0[first DOF of control
 * c's group], active_lower[c], active_upper[c]) -- a q0 off the coupling manifold is projected onto it this way, for fixed controls
 * too.  p_f(u): world position of finger f's site (site_parent, site_p).  With frame == 1 the targets are mapped to world once,
 * through the pose of site 0 at u0; the base is fixed in that mode.  Per iteration, with F the free controls and J_f the
 * 3 x |F| Jacobian of p_f with respect to u:
 *     A = sum_f w_f J_f^T J_f + lambda^2 I,   b = sum_f w_f J_f^T (t_f - p_f)     (fingers summed in the order f = 0..4)
 *     delta = A^-1 b  (Cholesky, no pivoting),   s = min(1, max_step / max_c |delta_c|),
 *     u_F <- clamp(u_F + s delta, active_lower, active_upper).
 * After `iters` iterations: controls = u, q_out = q(u), residual[f] = |t_f - p_f(u)| (unweighted, all five fingers, those with
 * weight 0 included).  A row's result depends on that row alone and is reproducible bit for bit.
 * UNITS.  The base slides (controls 0-2, metres) and base rotations (3-5, radians) share the one lambda and the one max_step with
 * the finger controls (radians): with the base free, lambda damps a metre of slide as much as a radian of rotation.
 *
 * targets (k, 5, 3) f32; controls (k, 18) f32, required; q_out (k, 26) f32 or NULL; residual (k, 5) f32 or NULL.
 * The controls are what the action stage consumes: DexSimBuffers::raw_targets (custom action rule), or, through
 * action = 2 (u - lower) / (upper - lower) - 1, a policy-style action in DEXSIM_MODE_POSITION.
 *
 * DEXSIM_ERR_ARG (with a dexsim_last_error text; no device needed): NULL targets, controls or prm; sites or frame outside {0, 1};
 * free_mask == 0 or a bit at position 18 or above; frame == 1 with a base bit (0..5) set; iters outside [1, DEXSIM_IK_MAX_ITERS];
 * damping or max_step not positive; a negative or all-zero weight; a NULL handle; k <= 0; env_ids == NULL without q0 and
 * k != num_envs.  DEXSIM_ERR_NOT_BOUND before dexsim_bind. */
#define DEXSIM_IK_MAX_ITERS 64
typedef struct DexSimIK {
  int      sites;        /* 0 = fingertip sites (DexHandModel sites 1..5), 1 = fingerpad sites (6..10) */
  int      frame;        /* 0 = targets in the env's world frame, 1 = in the hand frame: the pose of site 0 (right_hand_base),
                            the frame of the obs keys fingertip_poses_hand / fingerpad_poses_hand */
  uint32_t free_mask;    /* bit c set: control c (0..17, order of active_lower) is an unknown; others keep their start value */
  int      iters;        /* [1, DEXSIM_IK_MAX_ITERS] */
  float    damping;      /* lambda > 0 */
  float    max_step;     /* > 0: largest |change| of any control in one iteration */
  float    weight[5];    /* >= 0 per finger, not all 0; 0 drops the finger from the objective */
} DexSimIK;
int dexsim_ik_struct_size(size_t* out);
int dexsim_solve_ik(dexsim_t h, const int64_t* env_ids, int k, const float* q0, const float* targets, const DexSimIK* prm,
                    float* controls, float* q_out, float* residual, void* stream);

/* ------------------------------------------------------------------ clearance queries: hand / box, hand / ground, finger / finger
 * "Is this configuration free of collision, and how far is each link from the object, the ground and the other fingers?" -- for
 * planners (checking the joint positions dexsim_solve_ik returns), reward shaping and pre-grasp logic (per-link clearances) and
 * grasp analysis (contact points and normals for J^T f with dexsim_body_jacobian).  The engine itself collides the hand with the box
 * and the ground only -- it models no hand self-collision -- and its manifold is sub-step scratch, not API; this call is the public,
 * exact counterpart.  One launch, stream-ordered, never synchronises, allocates nothing; a pure function of the persistent state
 * (arena fields q, box_pos, box_quat) or of the caller's overrides: it writes no arena word, API tensor, statistics word, counter or
 * the step stamp.
 *
 * ROWS and the Q OVERRIDE are those of dexsim_body_jacobian: with q == NULL row i is env env_ids[i] (NULL: env i, k == num_envs) and
 * a row whose id is outside [0, num_envs) leaves its output rows untouched; with q != NULL, a device (k, 26) array, env_ids is
 * ignored and k may be any positive number.
 * THE BOX of a row: box_pose, a device (k, 7) f32 array (centre xyz, quaternion xyzw), when it is given; otherwise the row's env
 * (box_pos, box_quat) when q == NULL and cfg.has_box; otherwise there is no box.  Edge length: box_size if it is > 0, else
 * cfg.box_size.  The quaternion is normalised by the call (a zero quaternion is the identity).
 * A row's result depends on that row alone and is reproducible bit for bit; a q / box_pose row equal to an env's state gives that
 * env's output bit for bit.
 *
 * OUTPUTS, f32, 16-byte aligned; any may be NULL, not all three.
 * cap_env (k, DEXSIM_NCAP, 2, 8): for capsule c in DexHandModel order, record 0 against the box, record 1 against the ground plane
 * z = 0.  Words of a record:
 *     0     signed distance d between the surfaces (negative: overlap)
 *     1-3   unit normal n, world frame, pointing from the other shape towards the capsule
 *     4-6   witness point p on the other shape's surface, world frame
 *     7     t in [0, 1], the axis parameter of the capsule's witness: the axis point cap_p0 + t (cap_p1 - cap_p0) is
 *           p + (d + r) n, the witness on the capsule's surface p + d n
 *   Without a box the box record is (+inf, 0, 0, 0, 0, 0, 0, 0).
 * self_min (k, DEXSIM_NPROX_GROUPS, 8): the closest pair of each group of the pair table: word 0 d; 1-3 n, pointing from capsule B
 *   to capsule A; 4-6 the witness on B's surface; 7 the integer bits of the pair's index in the pair table.  Ties go to the lowest
 *   pair index.
 * pair_dist (k, DEXSIM_NPROX_PAIRS): d of every pair.
 *
 * PAIR TABLE (dexsim_proximity_pair: a host table, no handle needed).  Capsules 0-2 are the palm's, capsule 3 + 3 f + l is link l of
 * finger f (l = 0 proximal, 1 middle, 2 distal): the capsule with cap_fslot == 3 f + l.  Groups 0-9 are the finger pairs (fa < fb)
 * in lexicographic order, nine pairs each: pair 9 g + 3 la + lb is A = link la of finger fa against B = link lb of finger fb.
 * Groups 10-14 pair the palm with finger f = group - 10, six pairs each: pair 90 + 6 f + 2 i + (lb - 1) is A = palm capsule i
 * against B = link lb in {1, 2} of finger f; the proximal link is left out because it overlaps the palm by construction.  Links of
 * one finger are never paired.  A model that does not have exactly three palm capsules and one capsule per finger link in that
 * order (cap_fslot) is refused at the call.
 *
 * GEOMETRY, to fp32 roundoff; nothing here is iterated.
 * Capsule / ground: d = min(z0, z1) - r; t = 0 or 1, the lower end of the axis (a tie: 0); n = (0, 0, 1); p = that end projected
 *   onto z = 0.
 * Capsule / box: in the box frame, with the axis P(t) = a + t e, the half edge hb and f(t) = |P - clamp(P, -hb, hb)|^2, the witness
 *   parameter t* is the minimiser of f over [0, 1], the smallest t where the minimum is a flat stretch.  It is computed in closed
 *   form (f' is piecewise linear and non-decreasing with at most six breakpoints, where a coordinate crosses +-hb).  Axis outside
 *   the box: d = sqrt(f(t*)) - r, n = the normalised excess P - clamp(P) rotated to the world, p = clamp(P(t*)) in world coordinates.
 *   Axis meeting the box (sqrt(f(t*)) <= 1e-6 m, the threshold of the engine's sphere / box routine): t* becomes the midpoint of the
 *   stretch of the axis inside the box (slab clipping); depth = min_i (hb - |P_i(t*)|), the first axis winning a tie; d = -depth - r;
 *   n = +- that axis of the box, the sign of P_i (+ at zero); p = P(t*) moved onto that face.  This is the engine's rule for a sphere
 *   whose centre is inside the box; it is NOT a true penetration depth (the least translation that separates the shapes).  Such
 *   records are the ones with d <= -r.
 * Capsule / capsule: the clamped closest points c_A = a0 + s e_A, c_B = b0 + t e_B of the two axes by the standard two-stage clamping
 *   (s from the unconstrained optimum, clamped; t optimal for that s, clamped; if t was clamped, s optimal for that t, clamped).
 *   Parallel axes (|e_A|^2 |e_B|^2 - (e_A . e_B)^2 <= 1e-12 |e_A|^2 |e_B|^2): the first s is 0.  An axis with |e|^2 <= 1e-18 is a
 *   point.  d = |c_A - c_B| - r_A - r_B, n = (c_A - c_B) / |c_A - c_B|, or (0, 0, 1) when the axis distance is below 1e-9 m.
 *
 * DEXSIM_ERR_ARG (with a dexsim_last_error text; no device needed): all three outputs NULL, a misaligned output, a non-finite
 * box_size, k <= 0, a NULL handle, env_ids == NULL without q and k != num_envs, a model outside the pair table's capsule order, a box
 * without a positive edge length (box_size <= 0 and cfg.box_size <= 0).  DEXSIM_ERR_NOT_BOUND before dexsim_bind. */
#define DEXSIM_NPROX_GROUPS 15
#define DEXSIM_NPROX_PAIRS 120
/* pair i of the pair table, 0 <= i < DEXSIM_NPROX_PAIRS: capsule A, capsule B, group */
int dexsim_proximity_pair(int i, int* cap_a, int* cap_b, int* group);
int dexsim_query_proximity(dexsim_t h, const int64_t* env_ids, int k, const float* q, const float* box_pose, float box_size,
                           float* cap_env, float* self_min, float* pair_dist, void* stream);

/* ------------------------------------------------------------------ inverse dynamics and bias accelerations
 * The velocity-dependent members of the family that dexsim_body_jacobian / dexsim_mass_matrix begin: what a joint-space computed-torque
 * or impedance controller (tau = M qdd + c + g) and an operational-space or fingertip-force controller (xdd = J qdd + Jdot qd)
 * need beyond J(q), M(q) and g(q).  Functions of (q, qd).  Both calls are stream-ordered, never synchronise and allocate nothing,
 * and neither writes any arena word, API tensor, statistics word, counter or the step stamp.
 *
 * ROWS are those of dexsim_body_jacobian.  q and qd are BOTH NULL or BOTH device (k, 26) row-major overrides in dof_state order.
 * Both NULL: row i is env env_ids[i] (NULL: env i, and k must be num_envs) with its current q and qd (arena); a row whose id is
 * outside [0, num_envs) leaves its output row untouched.  Both given: they take the place of the state, env_ids is ignored and k
 * may be any positive number; a row of (q, qd) equal to an env's current state gives that env's output bit for bit.  Exactly one
 * of q and qd NULL is an error.
 *
 * INVERSE DYNAMICS  tau (k, 26) f32, 4-byte aligned:
 *     tau = M(q) qdd + c(q, qd)                       flags == 0
 *     tau = M(q) qdd + c(q, qd) + g(q)                flags == DEXSIM_ID_GRAVITY
 * the generalized force (N on the slides, N m on the hinges) that produces the joint acceleration qdd at the state (q, qd) --
 * by one recursive Newton-Euler pass, M is never formed.  M and g are those of dexsim_mass_matrix: general symmetric link
 * inertias, cfg.gravity, NO armature, NO PD terms, no contact and no joint-limit forces (the integrator's M^ adds
 * diag(armature + h (kd + h kp)); a controller that wants the armature adds armature[j] * qdd[j] itself).  c(q, qd) is the
 * velocity-product (Coriolis and centrifugal) force: c_i = sum_jk (dM_ij/dq_k - 1/2 dM_jk/dq_i) qd_j qd_k.
 * qdd: an optional device (k, 26) array aligned with the OUTPUT rows on either row path (row i of qdd belongs to row i of tau,
 * whichever env that is); NULL means zero, and tau is then the bias force c [+ g].  At qd = 0 and qdd = NULL with the gravity
 * flag the result is the gravity output of dexsim_mass_matrix to roundoff.
 *
 * BIAS ACCELERATIONS  acc (k, nb, 6) f32, 4-byte aligned; bodies as for dexsim_body_jacobian (HOST array of nb hand-body indices,
 * NULL = all DEXSIM_NUM_HAND_BODIES in order, nb must then be DEXSIM_NUM_HAND_BODIES).  Words 0-2: world linear acceleration of
 * the body-frame origin, words 3-5: world angular acceleration, both at qdd = 0 and without gravity: Jdot(q, qd) qd.  Contract:
 * with jac of dexsim_body_jacobian for the same body, jac[i, b] @ qdd + acc[i, b] is the time derivative of
 * rigid_body_states[env, b, 7:13] for the joint acceleration qdd.  Body 0 (hand_mount, welded to the fixed spawn frame) is all
 * zeros; with only slides moving, or qd = 0, everything is zero.  The bodies ride on the joint frames rigid_body_states places
 * them on; a model whose body_parent says otherwise is refused.
 *
 * DEXSIM_ERR_ARG (with a dexsim_last_error text; no device needed, nothing is launched): NULL handle, k <= 0, env_ids == NULL
 * without overrides and k != num_envs, exactly one of q and qd NULL, flag bits other than DEXSIM_ID_GRAVITY, nb outside
 * [1, DEXSIM_NUM_HAND_BODIES], a body index out of range, bodies == NULL with nb != DEXSIM_NUM_HAND_BODIES, a NULL or misaligned
 * output.  DEXSIM_ERR_NOT_BOUND before dexsim_bind. */
#define DEXSIM_ID_GRAVITY 1   /* include the gravity force g(q) */
int dexsim_inverse_dynamics(dexsim_t h, const int64_t* env_ids, int k, const float* q, const float* qd, const float* qdd,
                            int flags, float* tau, void* stream);
int dexsim_body_bias_accel(dexsim_t h, const int64_t* env_ids, int k, const float* q, const float* qd, const int* bodies, int nb,
                           float* acc, void* stream);

/* ------------------------------------------------------------------ forward kinematics: body states, site poses, centroid
 * The configuration the queries above and below describe, for the same rows and overrides: the entry point and DEXSIM_FK_HAND_FRAME
 * are declared and documented in dexsim_fk.h, which is part of this header. */
#include "dexsim_fk.h"

/* ------------------------------------------------------------------ forward dynamics and mass-matrix solves
 * The inverse direction of the family: which joint acceleration a generalized force produces at (q, qd), and M(q)^-1 applied to
 * caller vectors without forming M -- what a planner that rolls candidate torques forward, an operational-space controller
 * (Lambda^-1 = J M^-1 J^T), an effective-mass or impulse-response query and a check of a computed-torque controller need.  M is
 * block-arrow (base block, five finger blocks, no finger-finger coupling): the fingers are eliminated, the 6 x 6 Schur complement
 * is factored by Cholesky and the result back-substituted, one launch, 26 words written per row and right-hand side.  Both calls
 * are stream-ordered, never synchronise and allocate nothing, and neither writes any arena word, API tensor, statistics word,
 * counter or the step stamp.  A row's result depends on that row alone and is reproducible bit for bit.
 *
 * FORWARD DYNAMICS  qdd (k, 26) f32, 4-byte aligned:
 *     qdd = (M(q) [+ A])^-1 (tau - c(q, qd) [- g(q)])
 * M, c and g are exactly those of dexsim_mass_matrix and dexsim_inverse_dynamics: general symmetric link inertias, cfg.gravity, no
 * PD terms, no contact and no joint-limit forces (a caller folds such forces into tau).  g is included with DEXSIM_FD_GRAVITY; the
 * call is then the inverse of dexsim_inverse_dynamics with DEXSIM_ID_GRAVITY.  DEXSIM_FD_ARMATURE solves with M + A,
 * A = diag(DexHandModel::armature): for the inverse a caller cannot add the armature afterwards, so the flag exists here.
 * ROWS and the (q, qd) overrides are those of dexsim_inverse_dynamics, word for word.  tau: an optional device (k, 26) array
 * aligned with the OUTPUT rows on either row path; NULL means zero, and qdd is then the free acceleration.
 *
 * MASS SOLVE  out (k, nrhs, 26) f32, 4-byte aligned:
 *     out[i, r, :] = (M(q_i) [+ A])^-1 rhs[i, r, :]          nrhs in [1, DEXSIM_MSOLVE_MAX_RHS]
 * A function of q only; DEXSIM_FD_ARMATURE is the only flag.  ROWS and the q override are those of dexsim_mass_matrix; rhs is a
 * device (k, nrhs, 26) array aligned with the output rows.  A row is factored once and solved for all nrhs right-hand sides; a
 * column does not depend on nrhs or on its position among the columns.  out == rhs (in place) is allowed, any other overlap is
 * undefined.  With rows of dexsim_body_jacobian as right-hand sides this gives M^-1 J^T, with 26 unit columns M^-1 itself.  With
 * qd = 0, flags 0 and tau = r, dexsim_forward_dynamics returns the bits of the mass solve of r with nrhs = 1.
 *
 * DEXSIM_ERR_ARG (with a dexsim_last_error text; no device needed, nothing is launched): NULL handle, k <= 0, env_ids == NULL
 * without overrides and k != num_envs, exactly one of q and qd NULL, unknown flag bits (DEXSIM_FD_GRAVITY on the mass solve is
 * one), nrhs outside its range, NULL rhs, a NULL or misaligned output.  DEXSIM_ERR_NOT_BOUND before dexsim_bind. */
#define DEXSIM_FD_GRAVITY 1    /* gravity acts on the hand (same value as DEXSIM_ID_GRAVITY) */
#define DEXSIM_FD_ARMATURE 2   /* solve with M + diag(DexHandModel::armature) */
#define DEXSIM_MSOLVE_MAX_RHS 32
int dexsim_forward_dynamics(dexsim_t h, const int64_t* env_ids, int k, const float* q, const float* qd, const float* tau,
                            int flags, float* qdd, void* stream);
int dexsim_mass_solve(dexsim_t h, const int64_t* env_ids, int k, const float* q, const float* rhs, int nrhs, int flags,
                      float* out, void* stream);

/* ------------------------------------------------------------------ derivatives of the inverse and the forward dynamics
 * The linearisation of the two calls above about a state: what a trajectory optimiser (iLQR / DDP), an LQR design about a pose,
 * a stability check of an impedance law and a model-based learner consume.  Analytic (the tangent of the Newton-Euler pass), not
 * finite differences: in fp32 differences of dexsim_inverse_dynamics have no step at which roundoff and truncation are both small.
 * Both calls are stream-ordered, never synchronise and allocate nothing, and neither writes any arena word, API tensor, statistics
 * word, counter or the step stamp.  A row's result depends on that row alone and is reproducible bit for bit.
 *
 * INVERSE-DYNAMICS DERIVATIVES  of tau(q, qd, qdd) = M(q) qdd + c(q, qd) [+ g(q)], exactly the function dexsim_inverse_dynamics
 * computes (no armature, no PD, no contact, no joint-limit terms), at fixed qdd:
 *     dtau_dq[i, c, r] = d tau_r / d q_c          dtau_dqd[i, c, r] = d tau_r / d qd_c
 * LAYOUT: every derivative output of this section is (k, 26, 26) f32, 4-byte aligned, DERIVATIVE-MAJOR: the 26 contiguous words
 * out[i, c, :] are the derivative of the WHOLE vector with respect to coordinate c.  As a matrix out[i] is the TRANSPOSE of the
 * Jacobian d tau / d q; the first-order change is sum_c out[i, c, :] dq_c.  This is the row layout of dexsim_mass_solve
 * (out[i, r, :] = one right-hand side), so the forward route below solves its 26 rows in place.
 * ROWS, the (q, qd) overrides, ids outside [0, num_envs) (their output rows are left untouched) and qdd (optional, aligned with
 * the OUTPUT rows, NULL = zero) are those of dexsim_inverse_dynamics, word for word; DEXSIM_ID_GRAVITY is the only flag.  Either
 * output may be NULL (it is then not computed; the other has the bits it has when both are given), not both.
 * STRUCTURAL ZEROS: the torque of a joint of finger f does not depend on (q, qd) of finger g != f; those 4 x 4 blocks are written
 * as +0.0, not left untouched.
 *
 * FORWARD-DYNAMICS DERIVATIVES  of qdd(q, qd, tau) = (M(q) [+ A])^-1 (tau - c(q, qd) [- g(q)]), the function
 * dexsim_forward_dynamics computes, at fixed tau; flags DEXSIM_FD_GRAVITY | DEXSIM_FD_ARMATURE with the same meaning:
 *     dqdd_dq = -(M [+ A])^-1 dtau_dq      dqdd_dqd = -(M [+ A])^-1 dtau_dqd      (dtau_* at the returned qdd; A is constant)
 * in the layout above: dqdd_dq[i, c, r] = d qdd_r / d q_c.  qdd (k, 26) is REQUIRED: it receives the forward-dynamics result (the
 * bits of dexsim_forward_dynamics) and is where the intermediate lives, since nothing is allocated.  Either derivative output may
 * be NULL, not both.  Three launches on the stream: forward dynamics into qdd, the negated inverse-dynamics derivatives at that
 * qdd, the mass solve of each output's 26 rows in place.  Contract: as numbers (-0 == +0) the result equals the negated
 * dexsim_mass_solve (nrhs = 26, same DEXSIM_FD_ARMATURE) of dexsim_inverse_dynamics_derivatives at the returned qdd with the same
 * gravity flag.  There is no third output: d qdd / d tau is (M [+ A])^-1, which dexsim_mass_solve with 26 unit columns gives.
 * ROWS, overrides and tau (optional, aligned with the output rows, NULL = zero) are those of dexsim_forward_dynamics.  The base's
 * gimbal lock (q4 = +-pi/2), where M is singular, makes these derivatives unbounded.
 *
 * DEXSIM_ERR_ARG (with a dexsim_last_error text; no device needed, nothing is launched): the lists of dexsim_inverse_dynamics and
 * dexsim_forward_dynamics, plus both derivative outputs NULL, a misaligned derivative output, and a NULL or misaligned qdd of the
 * forward call.  DEXSIM_ERR_NOT_BOUND before dexsim_bind. */
int dexsim_inverse_dynamics_derivatives(dexsim_t h, const int64_t* env_ids, int k, const float* q, const float* qd,
                                        const float* qdd, int flags, float* dtau_dq, float* dtau_dqd, void* stream);
int dexsim_forward_dynamics_derivatives(dexsim_t h, const int64_t* env_ids, int k, const float* q, const float* qd,
                                        const float* tau, int flags, float* qdd, float* dqdd_dq, float* dqdd_dqd, void* stream);

const char* dexsim_error_string(int code);
const char* dexsim_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* DEXSIM_H */
