// dexsim_l2.hip.inc -- fused per-env kernels for the reference's post/pre-physics tensor math.
//
//   k_actions : ActionProcessor.process_actions (action_processor.py:284-352) with the default rules
//               (default_rules.py:33-112), filters (rules.py:141-190) and coupling (:571-614);
//               ObservationEncoder.update_prev_actions (:287-296).  ~25 torch kernels -> 1.  Its body is actions_block,
//               the block that also opens the first physics launch of dexsim_step.
//   k_post    : StepProcessor.process_physics_step (step_processor.py:37-131) = ObservationEncoder
//               (observation_encoder.py:576-758) + BlindGraspingTask.get_task_observations / FSM
//               (blind_grasping_task.py:549-978) + termination (step_processor.py:133-181,
//               blind_grasping_task.py:1210-1364, termination_manager.py:120-278) + rewards
//               (reward_calculator.py:66-275, blind_grasping_task.py:980-1208).  ~300 torch kernels and
//               8 host syncs -> 1 kernel, 0 syncs.
//   k_reset   : DexHandBase.reset_idx (dexhand_base.py:743-803) as a masked kernel with a device Philox
//               stream instead of torch.rand (blind_grasping_task.py:449-547).
//   k_finalize: the cross-env means / rates of TerminationManager.evaluate and consecutive successes.

// HardwareMapping enum order -> primary DOF (hand_initializer.py:20-38, observation_encoder.py:496-574)
constexpr int kActiveFingerDof[12] = {8, 7, 6, 10, 12, 11, 16, 15, 20, 19, 24, 23};

// obs_all row of each obs_dict key (include/dexsim.h); O_<key>_last is the key's last row
enum {
#define X(name, dim) O_##name, O_##name##_last = O_##name + (dim) - 1,
  DEXSIM_OBS_KEYS(X)
#undef X
  O_end
};
static_assert(O_end == DEXSIM_OBS_ALL_DIM, "DEXSIM_OBS_ALL_DIM is not the sum of the DEXSIM_OBS_KEYS dims");
static_assert(O_object_pos == DEXSIM_OBS_BASE_TASK_DIM, "DEXSIM_OBS_BASE_TASK_DIM is not the row of object_pos");

// The words the current step accumulates into (parity of its stamp) were cleared during the previous step; this clears the
// other pair for the next one.  No launch clears a word that the same launch, or a concurrently running one, adds to.
DI void begin_step_counters(int* cnt, int stamp) {
  const int o = (stamp & 1) ^ 1;
  cnt[CNT_CONTACTS + o] = 0; cnt[CNT_HAND_CONTACTS + o] = 0;
}

// ActionProcessor.process_actions with the 18 action channels spread over 6 wavefronts (channel i on wave i / 3): per
// channel 3 loads, a dozen ALU ops and ~8 stores instead of ~60 loads and ~110 stores on one wave.  zero_targets (the
// pre-finalize_setup branch, action_processor.py:305-318): every target is 0, active_prev_targets keeps its value and no
// raw target is read; the actions rows, the action copy and the step counters as in the other mode.
DI void actions_block(const Arena& A, const ApiPtrs& T, const DevParams* __restrict__ P, const float* __restrict__ act,
                      int zero_targets, int N, int NR) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int e = blockIdx.x * 64 + lane;
  const DexSimConfig& C = P->cfg;
  const int na = C.num_actions;
  const bool real = e < NR;
  // start of a control step: clear the NEXT step's contact statistics words (see CNT_CONTACTS; the reset gate is a stamp)
  if (blockIdx.x == 0 && threadIdx.x == 0) begin_step_counters(T.counters, T.stamp);
  const int fs = C.policy_controls_base ? 6 : 0;
  if (wv == 0) {
    FLD(targets, kHeldDof) = 0.f;
    if (real && T.full_dof_targets) T.full_dof_targets[(size_t)e * 26 + kHeldDof] = 0.f;
  }
#pragma unroll
  for (int i = 0; i < 18; i++) {
    if (i / 3 != wv) continue;
    // action slot i (prev_actions / actions rows) and control channel i share the wave
    const float ai = (real && i < na) ? act[(size_t)e * na + i] : 0.f;
    const int ci = i < 6 ? i : fs + (i - 6);                       // action index that drives control i
    const bool driven = i < 6 ? (C.policy_controls_base != 0) : (C.policy_controls_fingers != 0);
    const float ac = (driven && real && ci < na) ? act[(size_t)e * na + ci] : 0.f;
    float raw = FLD(active_rule_targets, i);
    const float prev = FLD(active_prev_targets, i);
    FLD(actions, i) = ai;
    if (T.actions_copy && real && i < na) T.actions_copy[(size_t)e * na + i] = ai;   // DexHandBase.actions = actions.clone()
    if (T.raw_targets && !zero_targets) {   // host-side custom action rule already produced active_raw_targets
      raw = real ? T.raw_targets[(size_t)e * 18 + i] : raw;
    } else if (C.control_mode == DEXSIM_MODE_POSITION_DELTA) {
      if (driven) raw = prev + ac * C.max_deltas[i];
      raw = clampf(raw, C.active_lower[i], C.active_upper[i]);
    } else {
      if (driven) raw = (ac + 1.0f) * 0.5f * (C.active_upper[i] - C.active_lower[i]) + C.active_lower[i];
    }
    const float d = clampf(raw - prev, -C.max_deltas[i], C.max_deltas[i]);
    const float nxt = clampf(prev + d, C.active_lower[i], C.active_upper[i]);
    if (!zero_targets) FLD(active_prev_targets, i) = nxt;
    const float tgt = zero_targets ? 0.f : nxt;
    // coupling: the DOFs of control i's group, written out per slot (as a loop over the group, the scatter makes the physics
    // kernels load the field pointers again on every wave)
    const CouplingGroup& g = kCoupling[i];
#define PUT(k) do { const float t = tgt * g.scale[k]; FLD(targets, g.dof[k]) = t; \
                    if (real && T.full_dof_targets) T.full_dof_targets[(size_t)e * 26 + g.dof[k]] = t; } while (0)
    PUT(0);
    if (g.n > 1) PUT(1);
    if (g.n > 2) PUT(2);
#undef PUT
    FLD(prev_actions, i) = ai;
  }
}

__global__ __launch_bounds__(384) void k_actions(Arena A, ApiPtrs T, const DevParams* __restrict__ P, const float* __restrict__ act,
                                                 int zero_targets, int N, int NR) {
  actions_block(P->arena, T, P, act, zero_targets, N, NR);
}

// ------------------------------------------------------------------------------------------------- post
DI V3 site_pos(const Arena& A, int N, int e, int s) { return {FLD(site_pose, 7 * s), FLD(site_pose, 7 * s + 1), FLD(site_pose, 7 * s + 2)}; }
DI Q4 site_quat(const Arena& A, int N, int e, int s) {
  return {FLD(site_pose, 7 * s + 3), FLD(site_pose, 7 * s + 4), FLD(site_pose, 7 * s + 5), FLD(site_pose, 7 * s + 6)};
}
// Every obs_dict value of the wavefront's 64 envs is assembled in LDS as s_ob[env][row] (row stride DEXSIM_OBS_ALL_DIM + 1 =
// 393, odd: conflict-free both for the per-env writes and for the transposed reads), then flushed twice, both fully
// coalesced: SoA into obs_all (the obs_dict views) and row-major into obs_buf (N, O), whose 64 consecutive rows are
// one contiguous block in HBM.  (v1 wrote obs_buf with 158 stride-632-B stores per lane and read obs_all back from
// memory in a dependent loop: 57 us.)
#define OB_STRIDE (DEXSIM_OBS_ALL_DIM + 1)
#define OB(i) s_ob[lane * OB_STRIDE + (i)]

// ---- k_post, v3.  A single wavefront can keep at most 64 memory instructions in flight and a burst of row accesses
// costs it ~50 cycles per instruction on top of the ~2 us first-touch latency (scripts/micro/cold_loads.hip: 200 row
// loads take 14.3k cycles on one wave, 6.0k spread over four), and arena loads cannot be hoisted above arena stores
// (may-alias).  v2 ran the whole per-env body on wave 0 (~200 loads, ~190 stores: 32k cycles).  v3 splits it:
//   phase A  helper waves 1..W-1: the observation groups that are plain functions of a few arena rows (DOF state and
//            finite-difference velocity, contact bookkeeping, pose rows, copy rows, finger-velocity reward sums), each
//            written as "all loads, compute, LDS rows, stores"; wave 0 meanwhile loads the task / termination state
//   phase B  wave 0: task observations + FSM, termination, rewards -- reading the helper results back from the LDS
//            tile, writing the reward table into LDS
//   phase C  all waves: coalesced flush of obs_all, obs_buf and the reward table
// LDS staging behind the observation tile (word index x 64 lanes)
#define ST_PEN 0      /* joint-limit penalty sum (task 0)                 */
#define ST_FV2 1      /* sum of squared finger velocities (task 2)        */
#define ST_FA2 2      /* sum of squared finger velocity changes (task 2)  */
#define ST_RC 3       /* reward table: DEXSIM_NUM_REWROWS rows + total reward */
#define ST_WORDS (ST_RC + DEXSIM_NUM_REWROWS + 1)
#define ST(i) s_st[(i) * 64 + lane]
#define POST_NTASK 12

// helper task t (see k_post): observation_encoder.py:576-758 split by input group
DI void post_task(int t, const Arena& A, const DevParams* __restrict__ P, const int* __restrict__ cnt, float* s_ob, float* s_st,
                  int obs_only, int N) {
  const int lane = threadIdx.x & 63;
  const int e = blockIdx.x * 64 + lane;
  const DexSimConfig& C = P->cfg;
  const DexHandModel& M = P->model;
  const float cdt = C.control_dt;
  if (t == 0) {            // DOF positions, manual finite-difference velocity (:298-321), joint-limit penalty
    float q[26], pq[26];
#pragma unroll
    for (int i = 0; i < 26; i++) { q[i] = FLD(q, i); pq[i] = FLD(prev_dof_pos, i); }
    float vel[26];
#pragma unroll
    for (int i = 0; i < 26; i++) vel[i] = (q[i] - pq[i]) / cdt;   // prev_dof_pos := q is stored by the flush (phase C)
#pragma unroll
    for (int i = 0; i < 6; i++) { OB(O_base_dof_pos + i) = q[i]; OB(O_base_dof_vel + i) = vel[i]; }
#pragma unroll
    for (int i = 0; i < 12; i++) {
      OB(O_active_finger_dof_pos + i) = q[kActiveFingerDof[i]]; OB(O_active_finger_dof_vel + i) = vel[kActiveFingerDof[i]];
    }
    float pen = 0.f;
#pragma unroll
    for (int i = 0; i < 20; i++) {
      OB(O_all_finger_dof_pos + i) = q[6 + i]; OB(O_all_finger_dof_vel + i) = vel[6 + i];
      const float lo = M.lo[6 + i], hi = M.hi[6 + i];
      const float nrm = 2.0f * (q[6 + i] - lo) / (hi - lo) - 1.0f;
      pen += clampf(fabsf(nrm) - 0.8f, 0.f, 1.f);
    }
    ST(ST_PEN) = pen;
  } else if (t == 1) {     // contact forces of the 5 distal links: magnitude, binary, duration (:323-361)
    float cf[15], prevb[5], cdur[5];
    // refresh of the (N,5,3) gathered contact-force copy (tensor_manager.py:441-446); the obs-only pass of
    // DexHandBase.reset() runs before it and sees the previous copy (dexhand_base.py:811-817)
#pragma unroll
    for (int f = 0; f < 5; f++)
#pragma unroll
      for (int i = 0; i < 3; i++) cf[3 * f + i] = obs_only ? FLD(cf5, 3 * f + i) : FLD(cforce, 3 * (3 * f + 2) + i);
#pragma unroll
    for (int f = 0; f < 5; f++) { prevb[f] = FLD(prev_contact_binary, f); cdur[f] = FLD(contact_duration_steps, f); }
    if (!obs_only) {
#pragma unroll
      for (int i = 0; i < 15; i++) FLD(cf5, i) = cf[i];
    }
#pragma unroll
    for (int f = 0; f < 5; f++) {
      const V3 F = {cf[3 * f], cf[3 * f + 1], cf[3 * f + 2]};
      OB(O_contact_forces + 3 * f) = F.x; OB(O_contact_forces + 3 * f + 1) = F.y; OB(O_contact_forces + 3 * f + 2) = F.z;
      const float mag = norm(F);
      OB(O_contact_force_magnitude + f) = mag;
      const float cur = (mag > C.contact_binary_threshold) ? 1.f : 0.f;
      OB(O_contact_binary + f) = cur;
      const bool started = (cur == 1.f) && (prevb[f] == 0.f);
      const float ns = started ? 1.f : (cur == 1.f ? cdur[f] + 1.f : 0.f);
      FLD(contact_duration_steps, f) = ns;
      FLD(prev_contact_binary, f) = cur;
      OB(O_contact_duration + f) = ns * cdt;
    }
  } else if (t == 2) {     // finger velocity / acceleration reward sums (reward_calculator.py:66-221), engine velocities
    if (obs_only) return;
    float v[20], pv[20];
#pragma unroll
    for (int i = 0; i < 20; i++) { v[i] = FLD(qd, 6 + i); pv[i] = FLD(prev_finger_dof_vel, i); }
    const int first = cnt[CNT_RC_FIRST];
    float fv2 = 0.f, fa2 = 0.f;
#pragma unroll
    for (int i = 0; i < 20; i++) {
      fv2 += v[i] * v[i];
      const float d = v[i] - (first ? v[i] : pv[i]);
      fa2 += d * d;
      FLD(prev_finger_dof_vel, i) = v[i];
    }
    ST(ST_FV2) = fv2; ST(ST_FA2) = fa2;
  } else if (t == 3) {     // targets
    float tg[26];
#pragma unroll
    for (int i = 0; i < 26; i++) tg[i] = FLD(targets, i);
#pragma unroll
    for (int i = 0; i < 6; i++) OB(O_base_dof_target + i) = tg[i];
#pragma unroll
    for (int i = 0; i < 12; i++) OB(O_active_finger_dof_target + i) = tg[kActiveFingerDof[i]];
#pragma unroll
    for (int i = 0; i < 20; i++) OB(O_all_finger_dof_target + i) = tg[6 + i];
  } else if (t == 4) {     // previous actions
    float v[18];
#pragma unroll
    for (int i = 0; i < 18; i++) v[i] = FLD(prev_actions, i);
#pragma unroll
    for (int i = 0; i < 18; i++) OB(O_prev_actions + i) = v[i];
  } else if (t == 5) {     // previous / rule targets
    float v[18];
#pragma unroll
    for (int i = 0; i < 18; i++) v[i] = FLD(active_prev_targets, i);
#pragma unroll
    for (int i = 0; i < 18; i++) {
      OB(O_active_prev_targets + i) = v[i];
      // default pre-action rule = identity clone (rules.py:78-95); a host-side custom rule overwrites the
      // field before the next action stage
      FLD(active_rule_targets, i) = v[i];
      OB(O_active_rule_targets + i) = v[i];
    }
  } else if (t == 6) {     // hand pose rows
    const V3 hp = site_pos(A, N, e, 0);
    const Q4 hq = site_quat(A, N, e, 0);
    OB(O_hand_pose + 0) = hp.x; OB(O_hand_pose + 1) = hp.y; OB(O_hand_pose + 2) = hp.z;
    OB(O_hand_pose + 3) = hq.x; OB(O_hand_pose + 4) = hq.y; OB(O_hand_pose + 5) = hq.z; OB(O_hand_pose + 6) = hq.w;
    const float sh = 0.7071067811865476f;
    const Q4 al = qmul(hq, Q4{0.f, -sh, 0.f, sh});
    OB(O_hand_pose_arr_aligned + 0) = hp.x; OB(O_hand_pose_arr_aligned + 1) = hp.y; OB(O_hand_pose_arr_aligned + 2) = hp.z;
    OB(O_hand_pose_arr_aligned + 3) = al.x; OB(O_hand_pose_arr_aligned + 4) = al.y; OB(O_hand_pose_arr_aligned + 5) = al.z;
    OB(O_hand_pose_arr_aligned + 6) = al.w;
  } else {                 // t = 7..11: fingertip / fingerpad pose rows of finger t-7, world and hand frame (:831-986)
    const int f = t - 7;
    const V3 hp = site_pos(A, N, e, 0);
    const Q4 hq = site_quat(A, N, e, 0);
    const V3 pw0 = site_pos(A, N, e, 1 + f), pw1 = site_pos(A, N, e, 6 + f);
    const Q4 qw0 = site_quat(A, N, e, 1 + f), qw1 = site_quat(A, N, e, 6 + f);
#pragma unroll
    for (int sidx = 0; sidx < 2; sidx++) {
      const V3 pw = sidx ? pw1 : pw0;
      const Q4 qw = sidx ? qw1 : qw0;
      const int ow = (sidx ? O_fingerpad_poses_world : O_fingertip_poses_world) + 7 * f;
      const int oh = (sidx ? O_fingerpad_poses_hand : O_fingertip_poses_hand) + 7 * f;
      OB(ow + 0) = pw.x; OB(ow + 1) = pw.y; OB(ow + 2) = pw.z; OB(ow + 3) = qw.x; OB(ow + 4) = qw.y; OB(ow + 5) = qw.z; OB(ow + 6) = qw.w;
      const V3 ph = qrot_inv(hq, pw - hp);                 // coordinate_transforms.py:17-35
      const Q4 qh = qmul(qconj(hq), qw);                   // observation_encoder.py:971-974
      OB(oh + 0) = ph.x; OB(oh + 1) = ph.y; OB(oh + 2) = ph.z; OB(oh + 3) = qh.x; OB(oh + 4) = qh.y; OB(oh + 5) = qh.z; OB(oh + 6) = qh.w;
    }
  }
}

// wave 0's inputs that are not observation rows: issued in phase A, consumed in phase B
struct PostIn {
  int estep, sds, stage, sreason, freason[DEXSIM_NUM_FAIL], pcont[5], first;
  float tis, scd, cf[15], tipz[5];
  V3 bpos, blin, bF, ib, hv, hw, phv, phw, hp, pad[5];
};
DI void post_load(const Arena& A, const DevParams* __restrict__ P, const int* __restrict__ cnt, int obs_only, int N, int e, PostIn& in) {
  const bool blind = P->cfg.task == DEXSIM_TASK_BLIND_GRASPING;
  in.estep = FLD(episode_step, 0);
  in.hp = site_pos(A, N, e, 0);
#pragma unroll
  for (int f = 0; f < 5; f++) {
    in.pad[f] = site_pos(A, N, e, 6 + f);
    in.tipz[f] = FLD(site_pose, 7 * (1 + f) + 2);
#pragma unroll
    for (int i = 0; i < 3; i++) in.cf[3 * f + i] = obs_only ? FLD(cf5, 3 * f + i) : FLD(cforce, 3 * (3 * f + 2) + i);
  }
  in.bpos = in.blin = in.bF = in.ib = in.hv = in.hw = in.phv = in.phw = V3{0, 0, 0};
  in.sds = 0; in.stage = 1; in.tis = 0.f; in.scd = 0.f; in.sreason = 0; in.first = 0;
#pragma unroll
  for (int i = 0; i < DEXSIM_NUM_FAIL; i++) in.freason[i] = 0;
#pragma unroll
  for (int f = 0; f < 5; f++) in.pcont[f] = 0;
  if (blind) {
    in.bpos = {FLD(box_pos, 0), FLD(box_pos, 1), FLD(box_pos, 2)};
    in.blin = {FLD(box_lin, 0), FLD(box_lin, 1), FLD(box_lin, 2)};
    in.bF = {FLD(cforce, 3 * DEXSIM_FSLOT_BOX), FLD(cforce, 3 * DEXSIM_FSLOT_BOX + 1), FLD(cforce, 3 * DEXSIM_FSLOT_BOX + 2)};
    in.sds = FLD(success_duration_steps, 0);
    in.stage = FLD(current_stage, 0);
    in.tis = FLD(time_in_stage, 0);
    in.scd = FLD(stage_contact_duration, 0);
  }
  if (!obs_only) {
    if (blind) in.ib = {FLD(initial_box_pos, 0), FLD(initial_box_pos, 1), FLD(initial_box_pos, 2)};
    in.sreason = FLD(success_reason, 0);
#pragma unroll
    for (int i = 0; i < DEXSIM_NUM_FAIL; i++) in.freason[i] = FLD(failure_reason, i);
    in.hv = {FLD(hand_vel, 0), FLD(hand_vel, 1), FLD(hand_vel, 2)};
    in.hw = {FLD(hand_vel, 3), FLD(hand_vel, 4), FLD(hand_vel, 5)};
    in.first = cnt[CNT_RC_FIRST];
    in.phv = {FLD(prev_hand_vel, 0), FLD(prev_hand_vel, 1), FLD(prev_hand_vel, 2)};
    in.phw = {FLD(prev_hand_ang_vel, 0), FLD(prev_hand_ang_vel, 1), FLD(prev_hand_ang_vel, 2)};
#pragma unroll
    for (int f = 0; f < 5; f++) in.pcont[f] = FLD(prev_contacts, f);
  }
}

// The logic of wave 0 is split around the phase-A/phase-B barrier: post_logic_a needs only wave 0's own loads (PostIn) and
// so overlaps the helper waves' observation tasks; post_logic_b (rewards) also reads helper results from the LDS tile.
struct PostMid {
  int estep, stage, just2, just3, sds, grasp, thumb, others, crit_f2, crit_f3, t_succ, t_fail, t_tout, should_reset, sreason,
      freason[DEXSIM_NUM_FAIL], crit_s, crit_f[DEXSIM_NUM_FAIL];
  float minz, avg_hd, grasp_duration, padz[3], cmag[5];
  V3 centroid;
};

// phase A (wave 0): BlindGraspingTask.get_task_observations + FSM, termination
DI void post_logic_a(const Arena& A, const ApiPtrs& T, const DevParams* __restrict__ P, float* s_ob, const PostIn& in, PostMid& m,
                     int obs_only, int N, int NR) {
  const int lane = threadIdx.x;   // wave 0: lane == threadIdx.x
  const int e = blockIdx.x * 64 + threadIdx.x;
  const DexSimConfig& C = P->cfg;
  const float cdt = C.control_dt;
  const bool blind = C.task == DEXSIM_TASK_BLIND_GRASPING;
  const Stamps st = Stamps::begin(0);
  // own copies of the few inputs the helper waves also turn into observation rows (same arithmetic, same values)
  const V3 hp = in.hp;
  V3 pad[5];
  int cb[5];
  float tipz[5];
#pragma unroll
  for (int f = 0; f < 5; f++) {
    pad[f] = in.pad[f];
    tipz[f] = in.tipz[f];
    const V3 F = {in.cf[3 * f], in.cf[3 * f + 1], in.cf[3 * f + 2]};
    m.cmag[f] = norm(F);
    cb[f] = m.cmag[f] > C.contact_binary_threshold;
  }
  int estep = in.estep;
  const V3 bpos = in.bpos, blin = in.blin, bF = in.bF, ib = in.ib;
  int stage = in.stage, sreason = in.sreason, freason[DEXSIM_NUM_FAIL];
#pragma unroll
  for (int i = 0; i < DEXSIM_NUM_FAIL; i++) freason[i] = in.freason[i];
  OB(O_episode_time) = (float)estep * cdt;
  // ---- BlindGraspingTask.get_task_observations (+ FSM)
  V3 centroid = {0, 0, 0};
  int just2 = 0, just3 = 0, sds = 0, grasp = 0, thumb = 0, others = 0;
  float hand_to_obj = 0.f, avg_hd = 0.f, grasp_duration = 0.f;
  if (blind) {
    OB(O_object_pos + 0) = bpos.x; OB(O_object_pos + 1) = bpos.y; OB(O_object_pos + 2) = bpos.z;
    OB(O_object_vel + 0) = blin.x; OB(O_object_vel + 1) = blin.y; OB(O_object_vel + 2) = blin.z;
    float sumd = 0.f, sumh = 0.f, pdist[5];
#pragma unroll
    for (int f = 0; f < 5; f++) {
      pdist[f] = norm(pad[f] - bpos);
      const float hd = fabsf(pad[f].z - bpos.z);
      OB(O_finger_to_object_distances + f) = pdist[f]; sumd += pdist[f];
      OB(O_finger_to_object_height_diff + f) = hd; sumh += hd;
    }
    OB(O_avg_finger_to_object_distance) = sumd / 5.f;
    avg_hd = sumh / 5.f;
    OB(O_avg_finger_to_object_height_diff) = avg_hd;
    hand_to_obj = norm(hp - bpos);
    OB(O_hand_to_object_distance) = hand_to_obj;
    {
      int k = 0;
#pragma unroll
      for (int a = 0; a < 5; a++)
#pragma unroll
        for (int b = a + 1; b < 5; b++) OB(O_fingerpad_distances + k++) = norm(pad[a] - pad[b]);
    }
    centroid = {(pad[0].x + pad[1].x + pad[2].x) / 3.f, (pad[0].y + pad[1].y + pad[2].y) / 3.f, (pad[0].z + pad[1].z + pad[2].z) / 3.f};
    OB(O_first_three_fingerpad_centroid + 0) = centroid.x; OB(O_first_three_fingerpad_centroid + 1) = centroid.y;
    OB(O_first_three_fingerpad_centroid + 2) = centroid.z;
    // finger-box contact heuristic (:773-833); the box force is read live (contact_forces_all view)
    const bool box_has = norm(bF) > C.contact_binary_threshold;
    const float prox = (float)(1.7320508075688772 * (double)C.box_size / 2 * 1.2);
    int fb[5], nf = 0;
#pragma unroll
    for (int f = 0; f < 5; f++) { fb[f] = cb[f] && box_has && (pdist[f] < prox); nf += fb[f]; }
    thumb = fb[0]; others = fb[1] | fb[2] | fb[3] | fb[4]; grasp = thumb & others;
    OB(O_thumb_contact) = (float)thumb; OB(O_other_fingers_contact) = (float)others; OB(O_grasp_state) = (float)grasp;
    const int cond = (bpos.z > C.height_threshold) && (nf >= C.min_fingers_for_grasp);
    sds = cond ? in.sds + 1 : 0;
    FLD(success_duration_steps, 0) = sds;
    FLD(success_conditions_met, 0) = cond;
    grasp_duration = (float)sds * cdt;
    OB(O_grasp_duration) = grasp_duration;
    // stage FSM (:835-978)
    float tis = in.tis + cdt;
    float scd = in.scd;
    const int tao = cb[0] && (cb[1] | cb[2] | cb[3] | cb[4]);
    if (stage == 2) scd = tao ? scd + cdt : 0.f;
    const int s1done = (stage == 1) && (tis >= C.stage1_duration);
    const int s2done = (stage == 2) && ((scd >= C.stage2_contact_success_threshold) || (tis >= C.stage2_duration));
    just2 = s1done; just3 = s2done;
    if (s1done) stage = 2;
    if (s2done) stage = 3;
    if (s1done || s2done) { tis = 0.f; scd = 0.f; }
    FLD(current_stage, 0) = stage; FLD(time_in_stage, 0) = tis; FLD(stage_contact_duration, 0) = scd;
    FLD(just2, 0) = just2; FLD(just3, 0) = just3;
    OB(O_current_stage) = (float)stage;
    OB(O_time_in_stage) = tis;
    float prog = 0.f;
    if (stage == 1) prog = clampf(tis / C.stage1_duration, 0.f, 1.f);
    if (stage == 2) prog = clampf(tis / C.stage2_duration, 0.f, 1.f);
    if (stage == 3) prog = 1.f;
    OB(O_stage_progress) = prog;
  }

  st.mark<SG_POST_LOGIC>(A, N, 0, blockIdx.x * 64, PL_TASK_OBS);
  if (obs_only) return;

  // ---- episode progress, termination (step_processor.py:80-181)
  estep += 1;
  FLD(episode_step, 0) = estep;
  int crit_f[DEXSIM_NUM_FAIL] = {0, 0, 0, 0, 0}, crit_s = 0;
  float minz = tipz[0];
#pragma unroll
  for (int f = 1; f < 5; f++) minz = fminf(minz, tipz[f]);
  if (C.height_safety_enabled) crit_f[0] = (hp.z < C.handbase_threshold) || (minz < C.fingertip_threshold);
  if (blind) {
    crit_s = sds >= C.contact_duration_threshold_steps;
    crit_f[1] = hand_to_obj > C.max_box_distance;
    // _evaluate_pregrasp_quality (:1334-1364)
    int height_ok = 1;
#pragma unroll
    for (int f = 0; f < 3; f++) height_ok &= (fabsf(pad[f].z - bpos.z) <= C.height_tolerance);
    const int centroid_ok = norm(centroid - bpos) <= C.centroid_tolerance;
    const int stab_ok = (norm(bpos - ib) <= C.position_drift_tolerance) && (norm(blin) <= C.velocity_tolerance);
    crit_f[2] = just2 && !(height_ok && centroid_ok && stab_ok);
    crit_f[3] = just3 && !grasp;
    crit_f[4] = (stage == 3) && !grasp;
  }
  FLD(crit_success, 0) = crit_s;
  int es = 0, ef = 0;
  if (C.active_success_mask & 1) { sreason |= (!es && crit_s); FLD(success_reason, 0) = sreason; es |= crit_s; }
#pragma unroll
  for (int i = 0; i < DEXSIM_NUM_FAIL; i++) {
    FLD(crit_failure, i) = crit_f[i];
    if ((C.active_failure_mask >> i) & 1) { freason[i] |= (!ef && crit_f[i]); FLD(failure_reason, i) = freason[i]; ef |= crit_f[i]; }
  }
  const int timeout = estep >= C.episode_length - 1;
  const int should_reset = es | ef | timeout;
  const int t_succ = es & should_reset, t_fail = ef & !es & should_reset, t_tout = timeout & !es & !ef & should_reset;
  FLD(episode_success, 0) = es; FLD(episode_failure, 0) = ef;
  FLD(term_success, 0) = t_succ; FLD(term_failure, 0) = t_fail; FLD(term_timeout, 0) = t_tout;
  FLD(reset_flag, 0) = should_reset;

  m.estep = estep; m.stage = stage; m.just2 = just2; m.just3 = just3; m.sds = sds; m.grasp = grasp; m.thumb = thumb; m.others = others;
  m.t_succ = t_succ; m.t_fail = t_fail; m.t_tout = t_tout; m.should_reset = should_reset; m.sreason = sreason; m.crit_s = crit_s;
#pragma unroll
  for (int i = 0; i < DEXSIM_NUM_FAIL; i++) { m.freason[i] = freason[i]; m.crit_f[i] = crit_f[i]; }
  m.minz = minz; m.avg_hd = avg_hd; m.grasp_duration = grasp_duration; m.centroid = centroid;
  m.padz[0] = pad[0].z; m.padz[1] = pad[1].z; m.padz[2] = pad[2].z;
}

// phase B (wave 0): rewards (reward_calculator.py:66-275, blind_grasping_task.py:980-1208), API buffers, statistics
DI void post_logic_b(const Arena& A, const ApiPtrs& T, const DevParams* __restrict__ P, int* __restrict__ cnt, float* s_ob, float* s_st,
                     const PostIn& in, const PostMid& m, int N, int NR) {
  const int lane = threadIdx.x;
  const int e = blockIdx.x * 64 + threadIdx.x;
  const bool real = e < NR;
  const DexSimConfig& C = P->cfg;
  const bool blind = C.task == DEXSIM_TASK_BLIND_GRASPING;
  const Stamps st = Stamps::begin(0);
  const int estep = m.estep, stage = m.stage, just2 = m.just2, just3 = m.just3, grasp = m.grasp, thumb = m.thumb, others = m.others;
  const int t_succ = m.t_succ, t_fail = m.t_fail, t_tout = m.t_tout, should_reset = m.should_reset, sreason = m.sreason, crit_s = m.crit_s;
  int freason[DEXSIM_NUM_FAIL], crit_f[DEXSIM_NUM_FAIL];
#pragma unroll
  for (int i = 0; i < DEXSIM_NUM_FAIL; i++) { freason[i] = m.freason[i]; crit_f[i] = m.crit_f[i]; }
  const float minz = m.minz, avg_hd = m.avg_hd, grasp_duration = m.grasp_duration;
  const V3 centroid = m.centroid, bpos = in.bpos, blin = in.blin, ib = in.ib, hv = in.hv, hw = in.hw;
  const int first = in.first;
  float cmag[5];
  V3 tip[5];
#pragma unroll
  for (int f = 0; f < 5; f++) {
    cmag[f] = m.cmag[f];
    tip[f] = {OB(O_fingertip_poses_world + 7 * f), OB(O_fingertip_poses_world + 7 * f + 1), OB(O_fingertip_poses_world + 7 * f + 2)};
  }
  st.mark<SG_POST_LOGIC>(A, N, 0, blockIdx.x * 64, PL_TERMINATION);
  // ---- rewards
  float r[DEXSIM_NUM_REWARD_TERMS];
#pragma unroll
  for (int i = 0; i < DEXSIM_NUM_REWARD_TERMS; i++) r[i] = 0.f;
  r[DEXSIM_REW_alive] = 1.f;
  r[DEXSIM_REW_height_safety] = clampf(1.0f - expf(-(minz - 0.02f) * 20.f), 0.f, 1.f);
  const float fv2 = ST(ST_FV2), pen = ST(ST_PEN), fa2 = ST(ST_FA2);   // helper tasks 2, 0, 2
  r[DEXSIM_REW_finger_velocity] = expf(-0.1f * sqrtf(fv2));
  r[DEXSIM_REW_hand_velocity] = expf(-0.2f * norm(hv));
  r[DEXSIM_REW_hand_angular_velocity] = expf(-0.2f * norm(hw));
  r[DEXSIM_REW_joint_limit] = 1.0f - pen / 20.f;
  {
    const V3 phv = first ? hv : in.phv;
    const V3 phw = first ? hw : in.phw;
    r[DEXSIM_REW_finger_acceleration] = expf(-2.0f * sqrtf(fa2));
    r[DEXSIM_REW_hand_acceleration] = expf(-0.5f * norm(hv - phv));
    r[DEXSIM_REW_hand_angular_acceleration] = expf(-0.5f * norm(hw - phw));
    FLD(prev_hand_vel, 0) = hv.x; FLD(prev_hand_vel, 1) = hv.y; FLD(prev_hand_vel, 2) = hv.z;
    FLD(prev_hand_ang_vel, 0) = hw.x; FLD(prev_hand_ang_vel, 1) = hw.y; FLD(prev_hand_ang_vel, 2) = hw.z;
    float changes = 0.f;
#pragma unroll
    for (int f = 0; f < 5; f++) {
      const int c = cmag[f] > 0.1f;
      const int pc = first ? c : in.pcont[f];
      changes += (c != pc) ? 1.f : 0.f;
      FLD(prev_contacts, f) = c;
    }
    r[DEXSIM_REW_contact_stability] = expf(-changes);
  }
  if (blind) {
    const float s1 = stage == 1 ? 1.f : 0.f, s2 = stage == 2 ? 1.f : 0.f, s3 = stage == 3 ? 1.f : 0.f;
    r[DEXSIM_REW_s1_height_alignment] = expf(-C.height_alignment_decay * avg_hd) * s1;
    r[DEXSIM_REW_s1_centroid_positioning] = expf(-C.centroid_positioning_decay * norm(centroid - bpos)) * s1;
    r[DEXSIM_REW_s1_object_stability] = expf(-C.object_stability_decay * (norm(bpos - ib) + norm(blin))) * s1;
    const float z0 = m.padz[0], z1 = m.padz[1], z2 = m.padz[2], mean = (z0 + z1 + z2) / 3.f;
    const float var = ((z0 - mean) * (z0 - mean) + (z1 - mean) * (z1 - mean) + (z2 - mean) * (z2 - mean)) / 2.f;
    r[DEXSIM_REW_s1_finger_height_consistency] = expf(-C.first_three_height_consistency_decay * var) * s1;
    r[DEXSIM_REW_s1_thumb_rotation] = expf(-5.0f * fabsf(OB(O_all_finger_dof_pos) - 1.5707963267948966f)) * s1;
    r[DEXSIM_REW_s2_thumb_contact] = (float)thumb * s2;
    r[DEXSIM_REW_s2_other_fingers_contact] = (float)others * s2;
    r[DEXSIM_REW_s2_grasp_achievement] = (float)grasp * s2;
    float mind = norm(tip[0] - bpos);
#pragma unroll
    for (int f = 1; f < 5; f++) mind = fminf(mind, norm(tip[f] - bpos));
    const float half = C.box_size / 2.0f;
    r[DEXSIM_REW_s2_fingerpad_proximity] = expf(-C.fingerpad_proximity_decay * fmaxf(mind, half * C.proximity_min_distance_factor)) * s2;
    float bv2 = 0.f;
#pragma unroll
    for (int i = 0; i < 6; i++) { const float vb = OB(O_base_dof_vel + i); bv2 += vb * vb; }
    r[DEXSIM_REW_s2_base_stability] = expf(-C.base_stability_decay * sqrtf(bv2)) * s2;
    r[DEXSIM_REW_s3_object_height] = clampf((bpos.z - C.box_z) / (C.height_threshold - C.box_z), 0.f, 1.f) * s3;
    r[DEXSIM_REW_s3_grasp_maintenance] = (float)grasp * s3;
    r[DEXSIM_REW_s3_grasp_duration] = clampf(grasp_duration / C.contact_duration_threshold_s, 0.f, 1.f) * s3;
    r[DEXSIM_REW_s1_completion] = (just2 && !crit_f[2]) ? 1.f : 0.f;
    r[DEXSIM_REW_s2_completion] = (just3 && !crit_f[3]) ? 1.f : 0.f;
    r[DEXSIM_REW_penetration_penalty] = fmaxf(half * C.geometric_penetration_factor - mind, 0.f) * C.penetration_depth_scale;
  }
  st.mark<SG_POST_LOGIC>(A, N, 0, blockIdx.x * 64, PL_REWARD_TERMS);
  float total = 0.f;
#pragma unroll
  for (int i = 0; i < DEXSIM_NUM_REWARD_TERMS; i++) {
    const float wgt = C.reward_weight[i], wr = r[i] * wgt;
    ST(ST_RC + i) = r[i];
    ST(ST_RC + DEXSIM_REWROW_WEIGHTED + i) = wr;
    if (wgt != 0.f) total += wr;
  }
  ST(ST_RC + DEXSIM_REWROW_TOTAL) = total;
  const float ts = t_succ ? C.success_reward : 0.f, tf = t_fail ? -C.failure_penalty : 0.f, tt = t_tout ? -C.timeout_penalty : 0.f;
  ST(ST_RC + DEXSIM_REWROW_TERM_RAW + 0) = (float)t_succ;
  ST(ST_RC + DEXSIM_REWROW_TERM_RAW + 1) = (float)t_fail;
  ST(ST_RC + DEXSIM_REWROW_TERM_RAW + 2) = (float)t_tout;
  ST(ST_RC + DEXSIM_REWROW_TERM_W + 0) = ts; ST(ST_RC + DEXSIM_REWROW_TERM_W + 1) = tf; ST(ST_RC + DEXSIM_REWROW_TERM_W + 2) = tt;
  const float rew = total + ts + tf + tt;
  ST(ST_RC + DEXSIM_NUM_REWROWS) = rew;
  if (real) {
    T.rew_buf[e] = rew;
    T.reset_buf[e] = (uint8_t)should_reset;
    if (T.sink_rew) T.sink_rew[e] = rew;
    if (T.sink_done) T.sink_done[e] = (uint8_t)should_reset;
    T.episode_step_count[e] = (int64_t)estep;
    T.episode_length[e] = (int64_t)estep;   // extras["episode_length"] = episode_step_count.clone() (:224)
    if (T.masks) {
      uint8_t* mk = T.masks + e;
      mk[(size_t)DEXSIM_MASK_SUCCESS * NR] = (uint8_t)t_succ;
      mk[(size_t)DEXSIM_MASK_FAILURE * NR] = (uint8_t)t_fail;
      mk[(size_t)DEXSIM_MASK_TIMEOUT * NR] = (uint8_t)t_tout;
      mk[(size_t)DEXSIM_MASK_SUCC_REASON * NR] = (uint8_t)sreason;
#pragma unroll
      for (int i = 0; i < DEXSIM_NUM_FAIL; i++) mk[(size_t)(DEXSIM_MASK_FAIL_REASON + i) * NR] = (uint8_t)freason[i];
    }
  }

  st.mark<SG_POST_LOGIC>(A, N, 0, blockIdx.x * 64, PL_REWARD_TABLE);
  // ---- cross-env statistics: wavefront ballot -> one atomic per wave and counter
  const int rs = real ? should_reset : 0;
  auto wave_count = [&](int pred, int slot) {
    const unsigned long long m = __ballot(pred);
    if (threadIdx.x == 0 && m) atomicAdd(&cnt[slot], __popcll(m));
  };
  wave_count(rs, CNT_NUM_RESETS);
  if (__any(rs) && threadIdx.x == 0) GPTR(cnt)[CNT_ANY_RESET] = T.stamp;   // every writer of this step stores the same value
  wave_count(real && crit_s, CNT_SUCC);
#pragma unroll
  for (int i = 0; i < DEXSIM_NUM_FAIL; i++) wave_count(real && crit_f[i], CNT_FAIL + i);
  wave_count(real && t_succ, CNT_TERM_SUCCESS);
  wave_count(real && t_fail, CNT_TERM_FAILURE);
  wave_count(real && t_tout, CNT_TERM_TIMEOUT);
  st.mark<SG_POST_LOGIC>(A, N, 0, blockIdx.x * 64, PL_STATS);
}

DI void reset_phase0(const Arena& A, const ApiPtrs& T, const DevParams* __restrict__ P, int N, int NR, int e);   // below

// the post tasks that read nothing the publication writes (DOF state, finger velocity sums, copy rows): run by the idle
// box wave of k_physics4 while waves 0-5 publish the last sub-step
DI void post_pre_tasks(const Arena& A, const DevParams* __restrict__ P, const int* __restrict__ cnt, float* s_ob, int N) {
  float* s_st = s_ob + 64 * OB_STRIDE;
#pragma unroll 1
  for (int t = 0; t < 6; t++)
    if ((POST_PRE_MASK >> t) & 1) post_task(t, A, P, cnt, s_ob, s_st, 0, N);
}

// helper task -> helper wave (of nh = W - 1 helpers); balanced for W = 8: no helper issues more than ~55 loads
__constant__ int c_post_task_wave[POST_NTASK] = {0, 1, 2, 3, 4, 4, 6, 2, 3, 5, 5, 6};
// ... and for W = 7 (the post block behind the last sub-step in k_physics4)
// (task 0 has already been run by the box wave while waves 0-5 published: POST_PRE_MASK; helper 0 takes tasks 1 and 3, helper 3
// task 2, helpers 4 and 5 one of the copy tasks 4, 5 next to their fingertip rows -- every helper stays under wave 0's ~10k cycles of phase A)
__constant__ int c_post_task_wave7[POST_NTASK] = {0, 0, 3, 0, 4, 5, 1, 1, 2, 3, 4, 5};

// W wavefronts per 64 envs (8 in the stand-alone launch).  fold_reset: the step path applies phase 0 of the in-step
// reset to the flagged envs right here, after the observations of the terminal state are assembled,
// instead of in a launch of its own.
DI void post_block(const Arena& A, const ApiPtrs& T, const DevParams* __restrict__ P, int* __restrict__ cnt, float* s_ob,
                   int obs_only, int fold_reset, int N, int NR, int done_mask) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6, nh = nw - 1;
  float* s_st = s_ob + 64 * OB_STRIDE;
  int* s_tab = (int*)(s_st + 64 * ST_WORDS);     // obs_buf column -> obs_all row, staged for the flush
  const int e = blockIdx.x * 64 + lane;
  const DexSimConfig& C = P->cfg;
  const Stamps st = Stamps::begin(0);
  // ---- phase A
  PostIn in;
  PostMid mid;
  if (wv == 0) {
    post_load(A, P, cnt, obs_only, N, e, in);
    if (C.task != DEXSIM_TASK_BLIND_GRASPING) {
#pragma unroll 4
      for (int i = DEXSIM_OBS_BASE_TASK_DIM; i < DEXSIM_OBS_ALL_DIM; i++) OB(i) = 0.f;
    }
    post_logic_a(A, T, P, s_ob, in, mid, obs_only, N, NR);
  } else {
    if (wv == nw - 1)
      for (int i = lane; i < C.num_obs; i += 64) s_tab[i] = P->obs_col_row[i];
#pragma unroll 1
    for (int t = 0; t < POST_NTASK; t++)
      if (!((done_mask >> t) & 1) && (nw == 7 ? c_post_task_wave7[t] : c_post_task_wave[t] % nh) == wv - 1)
        post_task(t, A, P, cnt, s_ob, s_st, obs_only, N);
  }
  st.mark<SG_POST>(A, N, wv, blockIdx.x * 64, POST_A);
  __syncthreads();
  // ---- phase B: wave 0 runs the reward / bookkeeping logic (it reads the tile, it does not write it); the observation
  // tile has been complete since the barrier above, so the helper waves flush it meanwhile, with 16-byte accesses.  A
  // wavefront keeps at most 64 memory instructions in flight against a ~2 us store round trip, so the flush time is set
  // by the NUMBER of store instructions per wave, not by bytes:
  // obs_all rows: one instruction = 4 rows x 64 envs (16 lanes x 4 consecutive envs per row);
  // obs_buf (N, O) row-major = concatenation of the configured keys (observation_encoder.py:783-829): the 64 rows of the
  // workgroup are one contiguous, 16-byte aligned block of 64*O floats, copied as float4 chunks.
  // (Round 1 flushed everything behind phase B: ~7k cycles of a 27k-cycle block.)
  const int r4 = lane >> 4, l16 = lane & 15;
  if (wv == 0) {
    if (!obs_only) post_logic_b(A, T, P, cnt, s_ob, s_st, in, mid, N, NR);
    if (fold_reset && e < NR && GPTR(A.reset_flag)[e] != 0) reset_phase0(A, T, P, N, NR, e);
  } else {
    const float* src = s_ob + (4 * l16) * OB_STRIDE + r4;
    // (obs_dict mode "policy", dexsim_set_obs_dict_mode: the rows behind obs_dict are not materialised -- 1 568 B per env and step
    // that a training loop never reads; the policy keys are served from obs_buf)
    if (!T.skip_obs_all)
    for (int g = wv - 1; g < DEXSIM_OBS_ALL_DIM / 4; g += nh) {      // DEXSIM_OBS_ALL_DIM is a multiple of 4
      const int row = 4 * g + r4;
      const f4 v = {src[4 * g], src[4 * g + OB_STRIDE], src[4 * g + 2 * OB_STRIDE], src[4 * g + 3 * OB_STRIDE]};
      st4_global(A.obs_all + (size_t)row * N + blockIdx.x * 64 + 4 * l16, v);
    }
    for (int g = wv - 1; g < 7; g += nh) {                           // prev_dof_pos := q (26 rows), from the q rows of the tile
      const int row = 4 * g + r4;
      if (row < 26) {
        const int ob = row < 6 ? O_base_dof_pos + row : O_all_finger_dof_pos + row - 6;
        const float* sq = s_ob + (4 * l16) * OB_STRIDE + ob;
        st4_global(A.prev_dof_pos + (size_t)row * N + blockIdx.x * 64 + 4 * l16, f4{sq[0], sq[OB_STRIDE], sq[2 * OB_STRIDE], sq[3 * OB_STRIDE]});
      }
    }
    const int O = C.num_obs;
    const int e0 = blockIdx.x * 64;
    const int nreal = min(64, NR - e0);
    const int total = nreal * O;                 // floats of this workgroup's block of obs_buf
    const unsigned magic = P->obs_div_magic;
    float* dst = T.obs_buf + (size_t)e0 * O;     // e0 * O * 4 bytes: multiple of 256
    float* dst2 = (T.sink_obs && !obs_only) ? T.sink_obs + (size_t)e0 * O : nullptr;
    for (int t4 = 4 * ((int)threadIdx.x - 64); t4 < total; t4 += 4 * ((int)blockDim.x - 64)) {
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int idx = min(t4 + j, total - 1);
        const int el = (int)__umulhi((unsigned)idx, magic);
        const int c = idx - el * O;
        v[j] = s_ob[el * OB_STRIDE + s_tab[c]];
      }
      if (t4 + 3 < total) {
        st4_global(dst + t4, f4{v[0], v[1], v[2], v[3]});
        if (dst2) st4_global(dst2 + t4, f4{v[0], v[1], v[2], v[3]});
      } else {
        for (int j = 0; j < 4 && t4 + j < total; j++) { dst[t4 + j] = v[j]; if (dst2) dst2[t4 + j] = v[j]; }
      }
    }
  }
  st.mark<SG_POST>(A, N, wv, blockIdx.x * 64, POST_B);   // (helpers: observation flush issued)
  __syncthreads();
  // ---- phase C: the reward table wave 0 has just written (rows + the total reward row), all waves
  if (!obs_only) {
    for (int g = wv; g < (DEXSIM_NUM_REWROWS + 1 + 3) / 4; g += nw) {
      const int row = 4 * g + r4;
      if (row <= DEXSIM_NUM_REWROWS) {
        const float* sr = s_st + (ST_RC + row) * 64 + 4 * l16;
        const f4 v = {sr[0], sr[1], sr[2], sr[3]};
        float* dst = row < DEXSIM_NUM_REWROWS ? A.rew_comp + (size_t)row * N : A.rew;
        st4_global(dst + blockIdx.x * 64 + 4 * l16, v);
      }
    }
  }
  st.mark<SG_POST>(A, N, wv, blockIdx.x * 64, POST_ROWS);
  st.mark<SG_POST>(A, N, wv, blockIdx.x * 64, POST_OBS);
}

#define POST_LDS_BYTES ((64 * OB_STRIDE + 64 * ST_WORDS + DEXSIM_OBS_ALL_DIM) * sizeof(float))
__global__ __launch_bounds__(512) void k_post(Arena A, ApiPtrs T, const DevParams* __restrict__ P, int* __restrict__ cnt,
                                              int obs_only, int fold_reset, int N, int NR) {
  extern __shared__ float s_post[];
  // the field pointers are read on demand through the scalar cache (P->arena): pinning the by-value copy across the
  // task loop cost 1.1 kB/lane of scratch spills
  post_block(P->arena, T, P, cnt, s_post, obs_only, fold_reset, N, NR, 0);
}

DI void finalize_stats(const ApiPtrs& T, const DevParams* __restrict__ P, int NR) {
  int* cnt = T.counters;
  float* st = T.stats;
  const DexSimConfig& C = P->cfg;
  // rates and means as correctly rounded quotients (count == NR must give exactly 1, like the reference's tensor.float().mean()):
  // the library is built with the faster <= 2.5 ulp fp32 division (build.py), so divide in double (one thread, once per step)
  auto mean = [&](int count) { return (float)((double)count / (double)NR); };
  st[DEXSIM_STAT_SUCC_MEAN] = mean(cnt[CNT_SUCC]);
  for (int i = 0; i < DEXSIM_NUM_FAIL; i++) st[DEXSIM_STAT_FAIL_MEAN + i] = mean(cnt[CNT_FAIL + i]);
  st[DEXSIM_STAT_SUCCESS_RATE] = mean(cnt[CNT_TERM_SUCCESS]);
  st[DEXSIM_STAT_FAILURE_RATE] = mean(cnt[CNT_TERM_FAILURE]);
  st[DEXSIM_STAT_TIMEOUT_RATE] = mean(cnt[CNT_TERM_TIMEOUT]);
  int cs = cnt[CNT_TERM_SUCCESS] > 0 ? cnt[CNT_CONSECUTIVE] + 1 : 0;   // termination_manager.py:323-339
  if (cs > C.max_consecutive_successes) cs = C.max_consecutive_successes;
  cnt[CNT_CONSECUTIVE] = cs;
  st[DEXSIM_STAT_CONSECUTIVE_SUCCESSES] = (float)cs;
  st[DEXSIM_STAT_NUM_RESETS] = (float)cnt[CNT_NUM_RESETS];
  st[DEXSIM_STAT_PHYSICS_STEPS] = cnt[CNT_ANY_RESET] == T.stamp ? 2.f : 1.f;
  // contacts of the control step's main physics step (last sub-step); the words were filled by the ungated launch
  st[DEXSIM_STAT_MEAN_CONTACTS] = mean(cnt[CNT_CONTACTS + (T.stamp & 1)]);
  st[DEXSIM_STAT_MEAN_HAND_CONTACTS] = mean(cnt[CNT_HAND_CONTACTS + (T.stamp & 1)]);
  cnt[CNT_RC_FIRST] = 0;
  for (int i = CNT_SUCC; i <= CNT_NUM_RESETS; i++) cnt[i] = 0;
  if (T.sink_stats)   // the rollout keeps the per-step statistics too: reduced over the ranks once per rollout (rollout.py)
    for (int i = 0; i < DEXSIM_STAT_USED; i++) T.sink_stats[i] = st[i];
}

// ------------------------------------------------------------------------------------------------- reset
// mode 1: reset the envs listed in ids[0..k);  mode 2: reset envs 0..k;  mode 3: reset envs whose reset_flag is set, without the
// device-side gate (staged tests; the step path runs the in-step reset inside k_post and the gated physics launch)
// phase 0: TerminationManager.reset_tracking + ResetManager.reset_idx up to reset_targets;
// phase 1: ObservationEncoder.reset_observer_state (after the extra physics step).
// ObservationEncoder.reset_observer_state (after the extra physics step)
DI void reset_phase1(const Arena& A, int N, int e) {
#pragma unroll
  for (int f = 0; f < 5; f++) { FLD(contact_duration_steps, f) = 0.f; FLD(prev_contact_binary, f) = 0.f; }
#pragma unroll
  for (int i = 0; i < 26; i++) FLD(prev_dof_pos, i) = 0.f;
#pragma unroll
  for (int i = 0; i < 18; i++) FLD(prev_actions, i) = 0.f;
}

// TerminationManager.reset_tracking + ResetManager.reset_idx up to reset_targets
DI void reset_phase0(const Arena& A, const ApiPtrs& T, const DevParams* __restrict__ P, int N, int NR, int e) {
  const DexSimConfig& C = P->cfg;
  FLD(episode_success, 0) = 0; FLD(episode_failure, 0) = 0; FLD(success_reason, 0) = 0;
#pragma unroll
  for (int i = 0; i < DEXSIM_NUM_FAIL; i++) FLD(failure_reason, i) = 0;
  FLD(episode_step, 0) = 0;
  T.episode_step_count[e] = 0;
  T.episode_length[e] = 0;   // extras["episode_length"] is cloned after the in-step resets (step_processor.py:113-115,224)
  if (T.masks) {   // reason masks are cleared in place for reset envs (termination_manager.py:352-356)
#pragma unroll
    for (int i = 0; i < DEXSIM_NUM_SUCC + DEXSIM_NUM_FAIL; i++) T.masks[(size_t)(DEXSIM_MASK_SUCC_REASON + i) * NR + e] = 0;
  }
  float q[26];
#pragma unroll
  for (int i = 0; i < 26; i++) q[i] = 0.f;
  const int rc = FLD(reset_count, 0);
  if (C.task == DEXSIM_TASK_BLIND_GRASPING) {
    float u[32];
    if (T.reset_samples) {
#pragma unroll
      for (int i = 0; i < DEXSIM_NRESET_SAMPLES; i++) u[i] = T.reset_samples[(size_t)e * DEXSIM_NRESET_SAMPLES + i];
    } else {
#pragma unroll
      for (int b = 0; b < 8; b++) {
        uint32_t x[4];
        philox4x32(x, (uint32_t)e, (uint32_t)rc, (uint32_t)b, 0u, C.seed, 0x5eedu);
#pragma unroll
        for (int i = 0; i < 4; i++) u[4 * b + i] = u01(x[i]);
      }
    }
    const float x = (u[0] * 2.f - 1.f) * C.box_xy_range, y = (u[1] * 2.f - 1.f) * C.box_xy_range;
    const float yaw = (u[2] * 2.f - 1.f) * 3.14159265358979323846f;
    if (!C.box_fixed) {   // (a static box stays where it was created)
      FLD(box_pos, 0) = x; FLD(box_pos, 1) = y; FLD(box_pos, 2) = C.box_z;
      FLD(initial_box_pos, 0) = x; FLD(initial_box_pos, 1) = y; FLD(initial_box_pos, 2) = C.box_z;
      FLD(box_quat, 0) = 0.f; FLD(box_quat, 1) = 0.f; FLD(box_quat, 2) = sinf(yaw / 2.f); FLD(box_quat, 3) = cosf(yaw / 2.f);
    }
#pragma unroll
    for (int i = 0; i < 3; i++) { FLD(box_lin, i) = 0.f; FLD(box_ang, i) = 0.f; }
    FLD(success_duration_steps, 0) = 0; FLD(success_conditions_met, 0) = 0;
    FLD(current_stage, 0) = 1; FLD(time_in_stage, 0) = 0.f; FLD(stage_contact_duration, 0) = 0.f;
    FLD(just2, 0) = 0; FLD(just3, 0) = 0;
#pragma unroll
    for (int i = 0; i < 3; i++) { q[i] = (u[3 + i] * 2.f - 1.f) * C.hand_translation_range; q[3 + i] = (u[6 + i] * 2.f - 1.f) * C.hand_rotation_range; }
#pragma unroll
    for (int i = 0; i < 20; i++) q[6 + i] = u[9 + i] * (i == 0 ? C.thumb_rotation_range : C.other_finger_range);
  }
  FLD(reset_count, 0) = rc + 1;
  FLD(wgen, 0) = DEXSIM_WGEN_NEXT(FLD(wgen, 0));   // the warm-start cache of the contact solver does not survive a teleport
#pragma unroll
  for (int i = 0; i < 26; i++) {
    FLD(q, i) = q[i]; FLD(qd, i) = 0.f; FLD(targets, i) = q[i];
    if (T.full_dof_targets) T.full_dof_targets[(size_t)e * 26 + i] = q[i];
  }
  // inverse coupling with the CPU last-writer-wins scatter (action_processor.py:616-666): a control takes the last DOF of
  // its group, divided by that DOF's scale
#pragma unroll
  for (int c = 0; c < 18; c++) {
    const CouplingGroup& g = kCoupling[c];
    FLD(active_prev_targets, c) = q[g.dof[g.n - 1]] / g.scale[g.n - 1];
  }
}

__global__ __launch_bounds__(64) void k_reset(Arena A, ApiPtrs T, const DevParams* __restrict__ P, const int64_t* __restrict__ ids, int k,
                                              int mode, int phase, int N, int NR) {
  int e = blockIdx.x * 64 + threadIdx.x;
  if (mode == 3) {
    if (e >= NR || FLD(reset_flag, 0) == 0) return;
  } else {
    if (e >= k) return;
    if (mode == 1) e = (int)ids[e];   // mode 2: all envs 0..k
    if (e < 0 || e >= NR) return;
  }
  if (phase == 1) reset_phase1(A, N, e);
  else reset_phase0(A, T, P, N, NR, e);
}

// ------------------------------------------------------------------------------------------------- finalize
__global__ void k_finalize(ApiPtrs T, const DevParams* __restrict__ P, int NR) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  finalize_stats(T, P, NR);
}

// start of a control step whose action stage did not run on the device (dexsim_reset, dexsim_begin_step)
__global__ void k_begin_step(int* cnt, int stamp) {
  if (threadIdx.x == 0 && blockIdx.x == 0) begin_step_counters(cnt, stamp);
}

// ------------------------------------------------------------------------------------------------- init / ingest
__global__ __launch_bounds__(64) void k_init(Arena A, ApiPtrs T, const DevParams* __restrict__ P, int N, int NR) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  const DexSimConfig& C = P->cfg;
  FLD(box_quat, 3) = 1.f;
  FLD(box_pos, 2) = C.box_z;
  FLD(initial_box_pos, 2) = C.box_z;
  if (C.box_fixed) {   // the harness's static contact-test box (examples/dexhand_test.py:950-1024): created at a fixed pose
#pragma unroll
    for (int i = 0; i < 3; i++) { FLD(box_pos, i) = C.box_fixed_pos[i]; FLD(initial_box_pos, i) = C.box_fixed_pos[i]; }
  }
  float mass = C.box_mass > 0.f ? C.box_mass : 1.f, mu = C.box_friction;
  if (C.dr_enabled) {
    uint32_t x[4];
    philox4x32(x, (uint32_t)e, 0u, 0u, 0u, C.dr_seed, 0xd12au);
    mass = C.dr_mass_lo + u01(x[0]) * (C.dr_mass_hi - C.dr_mass_lo);
    mu = C.dr_mu_lo + u01(x[1]) * (C.dr_mu_hi - C.dr_mu_lo);
  }
  FLD(box_mass, 0) = mass; FLD(box_mu, 0) = mu;
  FLD(current_stage, 0) = 1;
  if (e == 0) {
    for (int i = 0; i < DEXSIM_STAT_WORDS; i++) { T.counters[i] = 0; T.stats[i] = 0.f; }
    T.counters[CNT_RC_FIRST] = 1;
  }
}

// gym.set_dof_state_tensor_indexed / set_actor_root_state_tensor_indexed: AoS API tensor -> SoA arena
__global__ void k_ingest(Arena A, ApiPtrs T, const DevParams* __restrict__ P, const int64_t* __restrict__ ids, int k, int what,
                         int N, int NR) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  const int e = (int)ids[i];
  if (e < 0 || e >= NR) return;
  if (what == 0) {
    for (int j = 0; j < 26; j++) { FLD(q, j) = T.dof_state[((size_t)e * 26 + j) * 2]; FLD(qd, j) = T.dof_state[((size_t)e * 26 + j) * 2 + 1]; }
  } else if (P->cfg.has_box) {
    const float* b = T.root_state + ((size_t)e * 2 + 1) * 13;
    for (int j = 0; j < 3; j++) { FLD(box_pos, j) = b[j]; FLD(box_lin, j) = b[7 + j]; FLD(box_ang, j) = b[10 + j]; }
    for (int j = 0; j < 4; j++) FLD(box_quat, j) = b[3 + j];
  }
}
