"""ctypes mirrors of the structs in include/dexsim.h (the C-ABI drop-in boundary).

Kept in lock-step with the header; `check_struct_sizes` verifies sizeof() against the loaded library so
a drifted mirror fails loudly instead of corrupting memory.
"""
import ctypes as C

NJ, NBASE, NFINGER, NFJ, NACT = 26, 6, 5, 4, 18
NSITE, NCAP, NFSLOT, KMAX = 11, 18, 17, 24
NWKEY = 128     # DEXSIM_NWKEY: warm-start cache slots per env
FSLOT_PALM, FSLOT_BOX = 15, 16
NRESET_SAMPLES = 29
MAX_OBS_SEG = 40
NUM_HAND_BODIES = 37
OBS_ALL_DIM = 392
NUM_REWARD_TERMS = 26
NUM_COMMON_REWARD_TERMS = 10
REWROW_WEIGHTED, REWROW_TOTAL, REWROW_TERM_RAW, REWROW_TERM_W, NUM_REWROWS = 26, 52, 53, 56, 59
NUM_SUCC, NUM_FAIL = 1, 5
NUM_MASKS = 3 + NUM_SUCC + NUM_FAIL
MASK_SUCCESS, MASK_FAILURE, MASK_TIMEOUT, MASK_SUCC_REASON, MASK_FAIL_REASON = 0, 1, 2, 3, 3 + NUM_SUCC
STAT_WORDS = 64
STAT_USED = 20
STAT = dict(SUCC_MEAN=0, FAIL_MEAN=4, SUCCESS_RATE=12, FAILURE_RATE=13, TIMEOUT_RATE=14,
            CONSECUTIVE_SUCCESSES=15, NUM_RESETS=16, PHYSICS_STEPS=17, MEAN_CONTACTS=18, MEAN_HAND_CONTACTS=19)

TASK_BASE, TASK_BLIND_GRASPING = 0, 1
MODE_POSITION, MODE_POSITION_DELTA = 0, 1
STATE_VERSION = 1   # DEXSIM_STATE_VERSION: layout of a state record / state bank
STAGE = dict(DYNAMICS=0, SOLVE=1, PUBLISH=2, POST=3, RESET=4, FINALIZE=5, SUBSTEP=6, PHYSICS=7, STEP=8)

SUCCESS_CRITERIA = ["grasp_lift_success"]
FAILURE_CRITERIA = ["hitting_ground", "box_too_far", "stage1_pregrasp_failed",
                    "stage2_contact_failed", "stage3_grasp_lost"]

# camera sensors (include/dexsim.h: pixel model, scene record)
SEG_NONE, SEG_GROUND, SEG_BOX, SEG_CAPSULE0 = 0, 1, 2, 3
RENDER_AMBIENT = 0.35
RENDER_LIGHT = (2.0 / 7.0, 3.0 / 7.0, 6.0 / 7.0)          # unit vector towards the light, world frame
RENDER_PALETTE = ((150, 150, 140), (215, 150, 60), (200, 200, 210), (230, 80, 70), (80, 180, 90),
                  (70, 120, 230), (220, 200, 70), (180, 90, 200))   # ground, box, palm, finger 0..4
RENDER_BACKGROUND = (135, 170, 215)
RENDER_MAX_DIM = 4096
RCAP = dict(A=0, R=3, B=4, LEN=7, U=8, UO=11, O=12, INVR=15, N=16, CA=19, CB=20, LO=21, LU=22, R2=23)
RCAP_WORDS = 24
SCENE_WORDS = 52 + NCAP * RCAP_WORDS
RAY_MAX = 4096        # DEXSIM_RAY_MAX: rays per dexsim_raycast call
RAY_SKIP_PARENT = 1   # DEXSIM_RAY_SKIP_PARENT: a ray mounted on joint frame j does not test the capsules with cap_parent == j

f32, i32, u32 = C.c_float, C.c_int, C.c_uint32


class DexHandModel(C.Structure):
    _fields_ = [
        ("spawn_pos", f32 * 3), ("spawn_quat", f32 * 4),
        ("jtype", i32 * NJ),
        ("jqoff", (f32 * 4) * NJ), ("jpoff", (f32 * 3) * NJ), ("jaxis", (f32 * 3) * NJ),
        ("mass", f32 * NJ), ("com", (f32 * 3) * NJ), ("inertia", (f32 * 6) * NJ),
        ("kp", f32 * NJ), ("kd", f32 * NJ), ("armature", f32 * NJ), ("lo", f32 * NJ), ("hi", f32 * NJ),
        ("site_parent", i32 * NSITE), ("site_q", (f32 * 4) * NSITE), ("site_p", (f32 * 3) * NSITE),
        ("cap_parent", i32 * NCAP), ("cap_p0", (f32 * 3) * NCAP), ("cap_p1", (f32 * 3) * NCAP),
        ("cap_r", f32 * NCAP), ("cap_fslot", i32 * NCAP),
        ("hand_friction", f32),
        ("body_parent", i32 * NUM_HAND_BODIES), ("body_q", (f32 * 4) * NUM_HAND_BODIES),
        ("body_p", (f32 * 3) * NUM_HAND_BODIES), ("body_fslot", i32 * NUM_HAND_BODIES),
    ]


class DexSimConfig(C.Structure):
    _fields_ = [
        ("num_envs", i32), ("task", i32),
        ("dt", f32), ("substeps", i32), ("gravity", f32 * 3),
        ("num_position_iterations", i32),
        ("contact_offset", f32), ("rest_offset", f32), ("max_depenetration_velocity", f32),
        ("erp", f32), ("control_dt", f32), ("episode_length", i32), ("seed", u32),
        ("control_mode", i32), ("policy_controls_base", i32), ("policy_controls_fingers", i32),
        ("num_actions", i32),
        ("max_deltas", f32 * NACT), ("active_lower", f32 * NACT), ("active_upper", f32 * NACT),
        ("contact_binary_threshold", f32), ("num_obs", i32), ("n_obs_seg", i32),
        ("obs_seg_off", i32 * MAX_OBS_SEG), ("obs_seg_len", i32 * MAX_OBS_SEG),
        ("height_safety_enabled", i32), ("handbase_threshold", f32), ("fingertip_threshold", f32),
        ("active_success_mask", i32), ("active_failure_mask", i32),
        ("success_reward", f32), ("failure_penalty", f32), ("timeout_penalty", f32),
        ("max_consecutive_successes", i32),
        ("reward_weight", f32 * NUM_REWARD_TERMS),
        ("ground_friction", f32), ("has_box", i32),
        ("box_size", f32), ("box_mass", f32), ("box_friction", f32), ("box_xy_range", f32), ("box_z", f32),
        ("height_threshold", f32), ("contact_duration_threshold_s", f32),
        ("contact_duration_threshold_steps", i32), ("min_fingers_for_grasp", i32),
        ("max_box_distance", f32), ("stage1_duration", f32), ("stage2_duration", f32),
        ("hand_translation_range", f32), ("hand_rotation_range", f32),
        ("thumb_rotation_range", f32), ("other_finger_range", f32),
        ("stage2_contact_success_threshold", f32),
        ("height_alignment_decay", f32), ("centroid_positioning_decay", f32),
        ("object_stability_decay", f32), ("first_three_height_consistency_decay", f32),
        ("fingerpad_proximity_decay", f32), ("base_stability_decay", f32),
        ("geometric_penetration_factor", f32), ("proximity_min_distance_factor", f32),
        ("penetration_depth_scale", f32),
        ("height_tolerance", f32), ("centroid_tolerance", f32),
        ("position_drift_tolerance", f32), ("velocity_tolerance", f32),
        ("dr_enabled", i32), ("dr_mass_lo", f32), ("dr_mass_hi", f32), ("dr_mu_lo", f32), ("dr_mu_hi", f32),
        ("dr_seed", u32),
        ("box_fixed", i32), ("box_fixed_pos", f32 * 3),
        ("joint_limit_rows", i32), ("joint_limit_margin", f32),
    ]


class DexSimField(C.Structure):
    _fields_ = [("name", C.c_char * 40), ("rows", i32), ("is_int", i32), ("offset", C.c_size_t)]


class DexSimBuffers(C.Structure):
    _fields_ = [
        ("arena", C.c_void_p), ("stats", C.c_void_p), ("counters", C.c_void_p),
        ("obs_buf", C.c_void_p), ("rew_buf", C.c_void_p), ("reset_buf", C.c_void_p),
        ("episode_step_count", C.c_void_p), ("episode_length", C.c_void_p),
        ("dof_state", C.c_void_p), ("root_state", C.c_void_p),
        ("rigid_body_states", C.c_void_p), ("contact_forces_all", C.c_void_p),
        ("full_dof_targets", C.c_void_p), ("reset_samples", C.c_void_p),
        ("masks", C.c_void_p), ("raw_targets", C.c_void_p),
    ]


class DexSimCamera(C.Structure):
    _fields_ = [("width", i32), ("height", i32), ("hfov_deg", f32), ("near_clip", f32), ("far_clip", f32),
                ("parent_joint", i32), ("eye", f32 * 3), ("target", f32 * 3)]


IK_MAX_ITERS = 64   # DEXSIM_IK_MAX_ITERS
NPROX_GROUPS, NPROX_PAIRS = 15, 120   # DEXSIM_NPROX_GROUPS, DEXSIM_NPROX_PAIRS: the pair table of dexsim_query_proximity
ID_GRAVITY = 1   # DEXSIM_ID_GRAVITY: dexsim_inverse_dynamics includes the gravity force
FK_HAND_FRAME = 1   # DEXSIM_FK_HAND_FRAME: dexsim_forward_kinematics gives the site poses relative to site 0
FD_GRAVITY, FD_ARMATURE = 1, 2   # DEXSIM_FD_GRAVITY, DEXSIM_FD_ARMATURE: flags of dexsim_forward_dynamics / dexsim_mass_solve
MSOLVE_MAX_RHS = 32   # DEXSIM_MSOLVE_MAX_RHS


class DexSimIK(C.Structure):
    _fields_ = [("sites", i32), ("frame", i32), ("free_mask", u32), ("iters", i32), ("damping", f32), ("max_step", f32),
                ("weight", f32 * NFINGER)]


P, vp, sz, i64 = C.POINTER, C.c_void_p, C.c_size_t, C.c_int64

# every entry point include/dexsim.h declares and its argument types, in header order (tests/test_abi.py holds the names
# against the built library and the number of arguments against the header's declarations)
PROTOTYPES = {
    "dexsim_struct_sizes": [P(sz)],
    "dexsim_arena_layout": [P(DexSimConfig), P(DexSimField), i32, P(i32), P(sz)],
    "dexsim_obs_key_info": [i32, P(C.c_char_p), P(i32), P(i32)],
    "dexsim_reward_term_name": [i32, P(C.c_char_p)],
    "dexsim_body_name": [i32, P(C.c_char_p)],
    "dexsim_create": [P(DexSimConfig), P(DexHandModel), i32, P(vp)],
    "dexsim_destroy": [vp],
    "dexsim_bind": [vp, P(DexSimBuffers)],
    "dexsim_init_state": [vp, vp],
    "dexsim_process_actions": [vp, vp, i32, vp],
    "dexsim_begin_step": [vp, vp],
    "dexsim_physics_step": [vp, i32, vp],
    "dexsim_post_physics": [vp, i32, vp],
    "dexsim_step": [vp, vp, vp],
    "dexsim_reset_idx": [vp, vp, i32, vp],
    "dexsim_reset": [vp, vp],
    "dexsim_refresh_body_states": [vp, vp],
    "dexsim_set_dof_state_indexed": [vp, vp, i32, vp],
    "dexsim_set_root_state_indexed": [vp, vp, i32, vp],
    "dexsim_set_step_sink": [vp, vp, vp, vp],
    "dexsim_set_stats_sink": [vp, vp],
    "dexsim_set_obs_dict_mode": [vp, i32],
    "dexsim_set_phase_probe": [vp, vp],
    "dexsim_set_action_copy": [vp, vp],
    "dexsim_run_stage": [vp, i32, vp],
    "dexsim_time_stage": [vp, i32, i32, vp, P(f32)],
    "dexsim_step_timing": [vp, i32, P(f32), P(i32)],
    "dexsim_state_layout": [P(DexSimConfig), P(DexSimField), i32, P(i32), P(sz)],
    "dexsim_save_state": [vp, vp, vp, i32, vp, i64, vp],
    "dexsim_load_state": [vp, vp, vp, i32, vp, i64, vp],
    "dexsim_copy_envs": [vp, vp, vp, i32, vp],
    "dexsim_get_step_stamp": [vp, P(i32)],
    "dexsim_set_step_stamp": [vp, i32],
    "dexsim_camera_struct_size": [P(sz)],
    "dexsim_render_layout": [P(DexSimField), i32, P(i32), P(sz)],
    "dexsim_render": [vp, P(DexSimCamera), vp, vp, vp, i32, vp, vp, vp, vp, vp],
    "dexsim_body_jacobian": [vp, vp, i32, vp, P(i32), i32, vp, vp],
    "dexsim_mass_matrix": [vp, vp, i32, vp, vp, vp, vp],
    "dexsim_ik_struct_size": [P(sz)],
    "dexsim_solve_ik": [vp, vp, i32, vp, vp, P(DexSimIK), vp, vp, vp, vp],
    "dexsim_proximity_pair": [i32, P(i32), P(i32), P(i32)],
    "dexsim_query_proximity": [vp, vp, i32, vp, vp, f32, vp, vp, vp, vp],
    "dexsim_inverse_dynamics": [vp, vp, i32, vp, vp, vp, i32, vp, vp],
    "dexsim_body_bias_accel": [vp, vp, i32, vp, vp, P(i32), i32, vp, vp],
    "dexsim_forward_dynamics": [vp, vp, i32, vp, vp, vp, i32, vp, vp],
    "dexsim_mass_solve": [vp, vp, i32, vp, vp, i32, i32, vp, vp],
    "dexsim_inverse_dynamics_derivatives": [vp, vp, i32, vp, vp, vp, i32, vp, vp, vp],
    "dexsim_forward_dynamics_derivatives": [vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp],
    "dexsim_error_string": [i32],
    "dexsim_last_error": [],
}
EXPORTED_SYMBOLS = list(PROTOTYPES)
# the entry point include/dexsim_fk.h declares, the part of the header that dexsim.h includes (tests/test_forward_kinematics.py holds
# this table against that file and the built library as tests/test_abi.py holds the one above against dexsim.h)
FK_PROTOTYPES = {
    "dexsim_forward_kinematics": [vp, vp, i32, vp, vp, P(i32), i32, i32, vp, vp, vp, vp],
}
# the entry point include/dexsim_ray.h declares, a part of the header like dexsim_fk.h (tests/test_raycast.py holds this table against
# that file and the built library)
RAY_PROTOTYPES = {
    "dexsim_raycast": [vp, vp, i32, vp, vp, f32, vp, P(i32), i32, f32, f32, i32, vp, vp, vp],
}
ALL_PROTOTYPES = {**PROTOTYPES, **FK_PROTOTYPES, **RAY_PROTOTYPES}   # every entry point of the library: what the loader checks and declares


def declare_prototypes(lib):
    """Attach argtypes/restype for every entry point of include/dexsim.h and its parts dexsim_fk.h and dexsim_ray.h to a loaded CDLL."""
    for name, argtypes in ALL_PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = argtypes, i32
    lib.dexsim_error_string.restype = C.c_char_p
    lib.dexsim_last_error.restype = C.c_char_p
    return lib


def check_struct_sizes(lib):
    out = (C.c_size_t * 4)()
    lib.dexsim_struct_sizes(out)
    mine = [C.sizeof(DexHandModel), C.sizeof(DexSimConfig), C.sizeof(DexSimField), C.sizeof(DexSimBuffers)]
    if list(out) != mine:
        raise RuntimeError(f"dexsim ABI mismatch: library struct sizes {list(out)} != python mirrors {mine}")
    cam = C.c_size_t(0)
    lib.dexsim_camera_struct_size(C.byref(cam))
    if cam.value != C.sizeof(DexSimCamera):
        raise RuntimeError(f"dexsim ABI mismatch: DexSimCamera is {cam.value} bytes in the library, {C.sizeof(DexSimCamera)} in python")
    ik = C.c_size_t(0)
    lib.dexsim_ik_struct_size(C.byref(ik))
    if ik.value != C.sizeof(DexSimIK):
        raise RuntimeError(f"dexsim ABI mismatch: DexSimIK is {ik.value} bytes in the library, {C.sizeof(DexSimIK)} in python")
