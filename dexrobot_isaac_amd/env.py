"""DexHandEnv: the reference's L3 env surface (DexHandBase / VecTask) over libdexsim.

Mirrors reference dexhand_env/tasks/dexhand_base.py (step :893-942, reset :805-838, reset_idx :743-803,
get_observations_dict :948-956, observation_space/action_space :1150-1169) and the attribute names its callers
read.  The heavy lifting is one C-ABI call per method; this file only holds views, dict
bookkeeping and the hooks for host-side custom rules.  There is no CPU path in the product: `sim_device='cpu'`
raises (the reference's CPU pipeline is itself documented as broken for multi-env, docs/guide-debugging.md:309-353).
"""
import copy
import hashlib

import numpy as np
import torch

from . import _abi
from ._lib import DexSimError
from .config import (FINGER_COUPLING_MAP, HARDWARE_MAPPING, OBS_KEYS, REWARD_TERMS, build_sim_config,
                     obs_key_offsets)
from .spaces import Box


class EnvState:
    """A full snapshot of a DexHandEnv (DexHandEnv.get_state): the state bank with the record of every lane, the two global
    blocks (stats, counters), the step stamp, env.actions and the host-side state of the action-processor view -- plus what
    identifies the instance it fits: DEXSIM_STATE_VERSION, record_words, num_envs and a hash of the DexSimConfig / DexHandModel
    bytes.  Tensors stay on the device they were taken on; save() / load() move them through a plain dict of CPU tensors."""

    _TENSORS = ("bank", "stats", "counters", "actions")
    _INTS = ("version", "record_words", "num_envs", "capacity", "stamp")

    def __init__(self, version, record_words, num_envs, config_hash, capacity, stamp, bank, stats, counters, actions,
                 enabled_post_action_filters):
        self.version, self.record_words, self.num_envs = int(version), int(record_words), int(num_envs)
        self.config_hash, self.capacity, self.stamp = str(config_hash), int(capacity), int(stamp)
        self.bank, self.stats, self.counters, self.actions = bank, stats, counters, actions
        self.enabled_post_action_filters = [str(n) for n in enabled_post_action_filters]

    def to_dict(self):
        d = {k: getattr(self, k).detach().cpu() for k in self._TENSORS}
        d.update({k: int(getattr(self, k)) for k in self._INTS})
        d["config_hash"] = self.config_hash
        d["enabled_post_action_filters"] = list(self.enabled_post_action_filters)
        return d

    def save(self, path):
        torch.save(self.to_dict(), path)

    @classmethod
    def load(cls, path, device="cpu"):
        d = torch.load(path, map_location="cpu", weights_only=True)
        missing = [k for k in cls._TENSORS + cls._INTS + ("config_hash", "enabled_post_action_filters") if k not in d]
        if missing:
            raise DexSimError(f"EnvState.load: '{path}' is not an EnvState file (missing {missing})")
        return cls(**{k: d[k] for k in cls._INTS}, config_hash=d["config_hash"],
                   enabled_post_action_filters=d["enabled_post_action_filters"],
                   **{k: d[k].to(device) for k in cls._TENSORS})


class _PhysicsManagerView:
    """PhysicsManager attributes callers read (physics_manager.py:243-270)."""

    def __init__(self, sim_cfg):
        self.physics_dt = float(sim_cfg.dt)
        self.physics_steps_per_control_step = 2      # 1 main + 1 reset step, measured at init in the reference
        self.control_dt = float(sim_cfg.control_dt)
        self.auto_detected_physics_steps = True


class _ActionScalingView:
    """ActionScaling static helpers (scaling.py:28-99), torch-level, for callers that use them directly."""

    @staticmethod
    def scale_to_limits(actions, lower, upper):
        return (actions + 1.0) * 0.5 * (upper - lower) + lower

    @staticmethod
    def apply_velocity_deltas(prev_targets, actions, max_deltas):
        return prev_targets + actions * max_deltas

    @staticmethod
    def clamp_to_limits(targets, lower, upper):
        return torch.clamp(targets, lower, upper)

    @staticmethod
    def apply_velocity_clamp(new_targets, prev_targets, max_deltas):
        return prev_targets + torch.clamp(new_targets - prev_targets, -max_deltas, max_deltas)


class _ActionProcessorView:
    """ActionProcessor public API (action_processor.py:668-755) backed by the device action stage (actions_block: on the
    first physics launch of dexsim_step, or alone as k_actions)."""

    def __init__(self, env):
        self._env = env
        c, dev = env._sim_cfg, env.device
        self.action_control_mode = "position" if c.control_mode == _abi.MODE_POSITION else "position_delta"
        self.policy_controls_hand_base = bool(c.policy_controls_base)
        self.policy_controls_fingers = bool(c.policy_controls_fingers)
        self.NUM_BASE_DOFS, self.NUM_ACTIVE_FINGER_DOFS = 6, 12
        self.finger_coupling_map = FINGER_COUPLING_MAP
        self.max_deltas = torch.tensor(list(c.max_deltas), device=dev)
        self.active_lower_limits = torch.tensor(list(c.active_lower), device=dev)
        self.active_upper_limits = torch.tensor(list(c.active_upper), device=dev)
        mask = torch.zeros(18, dtype=torch.bool, device=dev)
        mask[:6] = self.policy_controls_hand_base
        mask[6:] = self.policy_controls_fingers
        self.active_target_mask = mask
        self.action_scaling = _ActionScalingView()
        self._pre_action_rule = None
        self._action_rule = None
        # post-action filters (rules.py:113-135): registry + enabled list.  The two built-ins run inside the action
        # kernel; as soon as a custom filter is enabled or a custom coupling rule is set, the whole action stage runs
        # on the host in torch (this file) and only its results are handed to the device (slow path, see env.step).
        self._post_action_filter_registry = {
            "velocity_clamp": lambda prev, rule, tgt: prev + torch.clamp(tgt - prev, -self.max_deltas, self.max_deltas),
            "position_clamp": lambda prev, rule, tgt: torch.clamp(tgt, self.active_lower_limits, self.active_upper_limits),
        }
        self._enabled_post_action_filters = ["velocity_clamp", "position_clamp"]   # dexhand_base.py:478-481
        self._coupling_rule = None
        # coupling table as index / scale tensors for the host path (constants.py:71-88)
        name_to_dof = {n: i for i, n in enumerate(env.model.dof_names)}
        ctrl, dof, scale = [], [], []
        for f, lst in FINGER_COUPLING_MAP.items():
            for jn, sc in lst:
                ctrl.append(6 + f); dof.append(name_to_dof[jn]); scale.append(sc)
        self._cpl_ctrl = torch.tensor(ctrl, device=dev)
        self._cpl_dof = torch.tensor(dof, device=dev)
        self._cpl_scale = torch.tensor(scale, device=dev, dtype=torch.float32)

    def _host_path(self):
        """True when the action stage cannot run in the HIP kernel: custom filter enabled or custom coupling rule."""
        return self._coupling_rule is not None or self._enabled_post_action_filters != ["velocity_clamp", "position_clamp"]

    def _default_action_rule(self, prev, rule_targets, actions):
        """default_rules.py:33-112 (position / position_delta), torch restatement for the host path."""
        raw = rule_targets.clone()
        na = actions.shape[1]
        fs = 6 if self.policy_controls_hand_base else 0
        a = torch.zeros(actions.shape[0], 18, device=actions.device, dtype=actions.dtype)
        if self.policy_controls_hand_base:
            a[:, :6] = actions[:, :6]
        if self.policy_controls_fingers:
            a[:, 6:] = actions[:, fs:fs + 12] if na >= fs + 12 else 0.0
        m = self.active_target_mask
        if self.action_control_mode == "position_delta":
            raw[:, m] = prev[:, m] + a[:, m] * self.max_deltas[m]
            raw = torch.clamp(raw, self.active_lower_limits, self.active_upper_limits)
        else:
            lo, hi = self.active_lower_limits, self.active_upper_limits
            raw[:, m] = ((a + 1.0) * 0.5 * (hi - lo) + lo)[:, m]
        return raw

    def _host_process_actions(self, actions):
        """ActionProcessor.process_actions on the host (action_processor.py:284-352): rule -> enabled filters in order
        -> coupling; writes the results into the device state the kernels read."""
        core = self._env._core
        prev, rule_t = self.active_prev_targets.clone(), self.active_rule_targets.clone()
        if self._action_rule is not None:
            config = {"control_mode": self.action_control_mode, "policy_controls_base": self.policy_controls_hand_base,
                      "policy_controls_fingers": self.policy_controls_fingers}
            raw = self._action_rule(prev, rule_t, actions, config)
        else:
            raw = self._default_action_rule(prev, rule_t, actions)
        nxt = raw
        for name in self._enabled_post_action_filters:
            fn = self._post_action_filter_registry.get(name)
            if fn is not None:                                   # rules.py:122-133: unknown names are skipped
                nxt = fn(prev, rule_t, nxt)
        if self._coupling_rule is not None:
            full = self._coupling_rule(nxt)
        else:
            full = torch.zeros(nxt.shape[0], 26, device=nxt.device, dtype=nxt.dtype)
            full[:, :6] = nxt[:, :6]
            full[:, self._cpl_dof] = nxt[:, self._cpl_ctrl] * self._cpl_scale
        core.field("active_prev_targets").copy_(nxt.t())
        core.field("targets").copy_(full.t())
        core.full_dof_targets.copy_(full)
        a18 = torch.zeros(actions.shape[0], 18, device=actions.device, dtype=actions.dtype)
        a18[:, :actions.shape[1]] = actions
        core.field("actions").copy_(a18.t())
        core.field("prev_actions").copy_(a18.t())
        core.begin_step()

    @property
    def active_prev_targets(self):
        return self._env._core.field("active_prev_targets").t()

    @property
    def active_rule_targets(self):
        return self._env._core.field("active_rule_targets").t()

    @property
    def full_dof_targets(self):
        return self._env._core.full_dof_targets

    @property
    def control_dt(self):
        return self._env.physics_manager.control_dt

    def set_pre_action_rule(self, rule):
        """rule(active_prev_targets (N,18), state={'obs_dict','env'}) -> active_rule_targets (rules.py:78-95)."""
        self._pre_action_rule = rule

    def set_action_rule(self, rule):
        """rule(active_prev_targets, active_rule_targets, actions, config) -> active_raw_targets (rules.py:97-111).
        Runs on the host in torch; the velocity/position clamps and the coupling still run in the HIP kernel."""
        self._action_rule = rule
        if rule is None:
            self._env._core.set_raw_targets(None)

    def register_post_action_filter(self, name, filter_fn):
        """filter_fn(active_prev_targets, active_rule_targets, active_targets) -> filtered (rules.py:113-135).  Like in the
        reference, registering does not enable: the name must also be in `_enabled_post_action_filters`
        (dexhand_base.py:255-261 extends that list with the task's `post_action_filters`)."""
        self._post_action_filter_registry[name] = filter_fn

    def set_coupling_rule(self, rule):
        """rule(active_targets (N,18)) -> full_dof_targets (N,26) (action_processor.py:698-705); None restores the table."""
        self._coupling_rule = rule

    def unscale_actions(self, actions):
        """actions in [-1, 1] -> physical units (action_processor.py:721-755)."""
        if self.action_control_mode == "position":
            return _ActionScalingView.scale_to_limits(actions, self.active_lower_limits[self.active_target_mask],
                                                      self.active_upper_limits[self.active_target_mask])
        return actions * self.max_deltas[self.active_target_mask]


class _ObservationEncoderView:
    """The obs_dict accessors callers use (observation_encoder.py:999-1665, the live subset)."""

    def __init__(self, env):
        self._env = env
        self.observation_keys = list(env.task_cfg["policy_observation_keys"])
        self.num_observations = int(env._sim_cfg.num_obs)
        self.raw_dof_name_to_index = {n: i for i, n in enumerate(env.model.dof_names)}
        self.control_name_to_index = {n: i for i, (n, _) in enumerate(HARDWARE_MAPPING)}
        idx, slices = 0, {}
        for k, (off, ln) in zip(self.observation_keys, env._obs_segments):
            slices[k] = (idx, idx + ln)
            idx += ln
        self.component_slice_indices = slices

    @property
    def task_states(self):
        c = self._env._core
        names = ["success_duration_steps", "success_conditions_met", "current_stage", "time_in_stage",
                 "stage_contact_duration", "just2", "just3"]
        out = {n: c.field(n)[0] for n in names}
        out["just_transitioned_to_stage2"] = out.pop("just2")
        out["just_transitioned_to_stage3"] = out.pop("just3")
        return out

    @property
    def obs_buf(self):
        return self._env.obs_buf

    def get_raw_finger_dof(self, dof_name, obs_type="pos", obs_data=None, env_idx=None):
        if dof_name not in self.raw_dof_name_to_index:
            raise ValueError(f"Unknown DOF name: {dof_name}. Available: {list(self.raw_dof_name_to_index.keys())}")
        if obs_data is None:
            raise ValueError("obs_data must be provided")
        key = {"pos": "all_finger_dof_pos", "vel": "all_finger_dof_vel", "target": "all_finger_dof_target"}.get(obs_type)
        if key is None:
            raise ValueError(f"Unknown obs_type: {obs_type}. Available: pos, vel, target")
        if not isinstance(obs_data, dict):
            raise ValueError(f"Raw finger DOF '{dof_name}' access requires obs_dict.")
        i = self.raw_dof_name_to_index[dof_name] - 6
        if i < 0:
            raise ValueError(f"DOF {dof_name} is not a finger DOF")
        data = obs_data[key][:, i]
        return data[env_idx].item() if env_idx is not None else data


class _PolicyObsDict(dict):
    """obs_dict in mode "policy" (env.obsDict: policy): the policy keys are views of obs_buf; every other key of the reference's
    obs_dict exists in the reference but is not materialised here -- asking for one is an error that says how to get it."""

    def __init__(self, views, all_keys):
        super().__init__(views)
        self._all_keys = set(all_keys)

    def copy(self):
        return _PolicyObsDict(dict(self), self._all_keys)

    def __missing__(self, key):
        if key in self._all_keys:
            raise KeyError(f"obs_dict['{key}'] is not materialised in env.obsDict = 'policy' mode (only the policy_observation_keys "
                           f"are: {sorted(self)}); create the env with cfg['env']['obsDict'] = 'all' (the default) to read it")
        raise KeyError(key)


class _TerminationManagerView:
    def __init__(self, env):
        self._env = env
        self.max_episode_length = int(env._sim_cfg.episode_length)
        self.max_consecutive_successes = int(env._sim_cfg.max_consecutive_successes)

    @property
    def consecutive_successes(self):
        return self._env._core.stats[_abi.STAT["CONSECUTIVE_SUCCESSES"]]

    @property
    def episode_success(self):
        return self._env._core.field("episode_success")[0].bool()

    @property
    def episode_failure(self):
        return self._env._core.field("episode_failure")[0].bool()


class _TaskView:
    def __init__(self, name):
        self.name = name


class ProximityResult:
    """What DexHandEnv.query_proximity returns: the three device tensors (None where not requested), the pair table and the names
    behind the capsule and group indices."""
    FINGER_NAMES = ("thumb", "index", "middle", "ring", "pinky")

    def __init__(self, model, pairs, cap_env=None, self_min=None, pair_dist=None):
        self.cap_env, self.self_min, self.pair_dist = cap_env, self_min, pair_dist
        self.pairs = torch.as_tensor(pairs, dtype=torch.int64).view(_abi.NPROX_PAIRS, 3)   # (capsule A, capsule B, group), host
        self._model = model

    def capsule_body(self, c):
        """Name of the rigid body capsule c belongs to (a row name of rigid_body_states)."""
        c = int(c)
        if not 0 <= c < _abi.NCAP:
            raise IndexError(f"capsule index must be in [0, {_abi.NCAP}), got {c}")
        slot = int(self._model.cap_fslot[c])
        return self._model.body_names[[int(s) for s in self._model.body_fslot].index(slot)]

    def group_fingers(self, g):
        """The two sides of group g: a pair of finger names, or ("palm", finger name)."""
        g = int(g)
        if not 0 <= g < _abi.NPROX_GROUPS:
            raise IndexError(f"group index must be in [0, {_abi.NPROX_GROUPS}), got {g}")
        if g >= 10:
            return ("palm", self.FINGER_NAMES[g - 10])
        fa, fb = [(a, b) for a in range(5) for b in range(a + 1, 5)][g]
        return (self.FINGER_NAMES[fa], self.FINGER_NAMES[fb])

    @property
    def min_pair(self):
        """(k, 15) int64: the pair-table index of every group's closest pair (word 7 of self_min)."""
        return self.self_min[..., 7].contiguous().view(torch.int32).to(torch.int64)


class DexHandEnv:
    """Vectorised DexHand environment on one MI355X (one process per GPU; shard envs across ranks)."""

    def __init__(self, cfg, task_name, rl_device, sim_device, graphics_device_id=0, headless=True, force_render=False,
                 video_config=None, domain_randomisation=None, hand_model=None, _core_factory=None):
        self.cfg = cfg
        self.env_cfg, self.task_cfg, self.sim_cfg = cfg["env"], cfg["task"], cfg["sim"]
        self.video_config = video_config
        self.headless, self.force_render = headless, force_render
        self.graphics_device_id = graphics_device_id
        # Env.__init__ device rule (vec_task.py:61-84): "cuda:k"/"gpu" => GPU pipeline, anything else => cpu
        split = str(sim_device).split(":")
        dev_type = split[0].lower()
        if "use_gpu_pipeline" in cfg.get("sim", {}):
            raise RuntimeError("The 'use_gpu_pipeline' config key is deprecated and must be removed. "
                               "GPU pipeline is now automatically determined from sim_device.")
        if dev_type in ("cuda", "gpu"):
            self.use_gpu_pipeline = True
            self.device = f"cuda:{int(split[1]) if len(split) > 1 else 0}"
        else:
            self.use_gpu_pipeline = False
            self.device = "cpu"
        self.rl_device = rl_device
        if torch.device(rl_device) != torch.device(self.device) and _core_factory is None:
            # TensorManager refuses wrapped tensors that are not on rl_device (tensor_manager.py:178-185)
            raise RuntimeError(f"Device mismatch: rl_device '{rl_device}' but simulation tensors live on '{self.device}'.")
        self.max_episode_length = self.env_cfg["episodeLength"]
        self.num_envs = int(self.env_cfg["numEnvs"])
        self.clip_obs = self.env_cfg.get("clipObservations", np.inf)      # read, never applied (vec_task.py:108-109)
        self.clip_actions = self.env_cfg.get("clipActions", np.inf)
        self.seed(cfg["train"]["seed"])

        # hand_model: a HandModel, e.g. dexrobot_isaac_amd.mjcf.load_mjcf(<dexhand021_right_simplified_floating.xml>);
        # None = the authored stand-in (the reference's MJCF submodule is absent offline)
        self._sim_cfg, self.model = build_sim_config(cfg, model=hand_model, dr=domain_randomisation)
        self._model_struct = self.model.to_struct()
        if _core_factory is None:
            from .core import DexSimCore
            if not self.use_gpu_pipeline:
                from ._lib import DexSimError
                raise DexSimError("sim_device='cpu' is not supported: dexsim is a HIP-only engine with no CPU fallback")
            self._core = DexSimCore(self._sim_cfg, self._model_struct, self.device)
        else:
            self._core = _core_factory(self._sim_cfg, self._model_struct, self.device)
        core = self._core
        self.task = _TaskView(task_name)
        self.physics_dt = float(self._sim_cfg.dt)
        self.dt = self.physics_dt
        self.physics_manager = _PhysicsManagerView(self._sim_cfg)
        self.physics_steps_per_control_step = 2
        self._num_observations = int(self._sim_cfg.num_obs)
        self._num_actions = int(self._sim_cfg.num_actions)
        self.num_states = 0
        self.num_dof = _abi.NJ
        self._obs_segments = [(int(self._sim_cfg.obs_seg_off[i]), int(self._sim_cfg.obs_seg_len[i]))
                              for i in range(int(self._sim_cfg.n_obs_seg))]
        # index contract the reference resolves through Isaac Gym name lookups (hand_initializer.py:439-588)
        self.base_joint_names = self.model.dof_names[:6]
        self.finger_joint_names = [n for n in self.model.dof_names[6:] if n != "r_f_joint3_1"]
        self.hand_local_rigid_body_index = self.model.hand_local_rigid_body_index
        self.hand_local_actor_index = 0
        self.fingertip_local_indices = self.model.fingertip_local_indices
        self.fingerpad_local_indices = self.model.fingerpad_local_indices
        self.contact_force_local_body_indices = self.model.body_indices(self.task_cfg["contact_force_bodies"])
        self.dof_props = torch.tensor(self.model.dof_props(), device=self.device)
        self.action_control_mode = self.task_cfg["controlMode"]
        self.policy_controls_hand_base = bool(self.task_cfg["policy_controls_hand_base"])
        self.policy_controls_fingers = bool(self.task_cfg["policy_controls_fingers"])
        self.action_processor = _ActionProcessorView(self)
        self.observation_encoder = _ObservationEncoderView(self)
        self.termination_manager = _TerminationManagerView(self)

        # buffers (initialization_manager.py:34-117): env-owned, returned by reference from step()
        self.obs_buf, self.states_buf = core.obs_buf, core.obs_buf
        self.rew_buf, self.reset_buf = core.rew_buf, core.reset_buf
        self.episode_step_count = core.episode_step_count
        self.actions = torch.zeros((self.num_envs, self._num_actions), device=self.device)
        self._actions_copy_bound = hasattr(core, "set_action_copy")     # (the CPU oracle stand-in of the tests has no sink)
        if self._actions_copy_bound:
            core.set_action_copy(self.actions)
        self.dof_state = core.dof_state
        self.dof_pos, self.dof_vel = core.dof_state[..., 0], core.dof_state[..., 1]
        self.actor_root_state_tensor = core.root_state
        self._build_views()

        # control-cycle measurement of the reference's __init__ (dexhand_base.py:270-320): zero targets,
        # one physics step, reset of every env (with its physics step); control_dt = 2 * sim.dt
        core.process_actions(self.actions, zero_targets=True)
        core.physics_step()
        core.reset_idx(torch.arange(self.num_envs, device=self.device))
        self._apply_pre_action_rule()
        # camera sensors (GraphicsManager.create_camera, graphics_manager.py:56-179).  A video_config with a `resolution`
        # creates the reference's fixed "video" camera, placed as VideoManager._position_camera places it
        # (video_manager.py:100-147): 75 deg, behind env 0, looking at the hand.
        self._cameras = {}
        if video_config and video_config.get("resolution") is not None:
            w, h = (int(v) for v in video_config["resolution"])
            back = max(1.5, 0.75 * float(self.env_cfg["envSpacing"]))
            self.create_camera("video", w, h, hfov_deg=75.0, eye=(-back, 0.0, 0.5), target=(0.0, 0.0, 0.15))
        self._initialization_complete = True

    # ------------------------------------------------------------------ construction helpers
    def seed(self, seed=None):                                   # vec_task.py:145-153
        if seed is None:
            return
        import random
        random.seed(seed)
        np.random.seed(seed)
        torch.manual_seed(seed)

    def _build_views(self):
        core, c = self._core, self._sim_cfg
        offs = obs_key_offsets()
        oa = core.field("obs_all")
        n_keys = len(OBS_KEYS) if c.task == _abi.TASK_BLIND_GRASPING else 23
        # env.obsDict (new key): "all" (default) = every key of the reference's obs_dict is materialised each step (392 SoA rows per
        # env); "policy" = only obs_buf is written and obs_dict serves the policy keys as views of it -- what a training loop
        # needs (dexsim_set_obs_dict_mode; 1 568 B per env and step less to write)
        self.obs_dict_mode = str(self.env_cfg.get("obsDict", "all"))
        if self.obs_dict_mode not in ("all", "policy"):
            raise ValueError(f"env.obsDict must be 'all' or 'policy', got '{self.obs_dict_mode}'")
        if self.obs_dict_mode == "policy" and hasattr(core, "set_obs_dict_mode"):
            core.set_obs_dict_mode(True)
            views = {k: self.obs_buf[:, a:b] for k, (a, b) in self.observation_encoder.component_slice_indices.items()}
            self.obs_dict = _PolicyObsDict(views, [k for k, _ in OBS_KEYS[:n_keys]])
        else:
            self.obs_dict_mode = "all"
            self.obs_dict = {}
        for name, dim in OBS_KEYS[:n_keys]:
            if self.obs_dict_mode != "all":
                break
            off, _ = offs[name]
            if name == "prev_actions":
                dim = int(c.num_actions)
            self.obs_dict[name] = oa[off:off + dim].t()          # (N, dim) view of the SoA rows
        rc = core.field("rew_comp")
        comps = {}
        for i, name in enumerate(REWARD_TERMS):
            if float(c.reward_weight[i]) != 0.0:                  # reward_calculator.py:255-270
                comps[name] = rc[i]
                comps[f"{name}_weighted"] = rc[_abi.REWROW_WEIGHTED + i]
        comps["total"] = rc[_abi.REWROW_TOTAL]
        for j, name in enumerate(("success", "failure_penalty", "timeout_penalty")):   # step_processor.py:204-219
            comps[f"termination_{name}"] = rc[_abi.REWROW_TERM_RAW + j]
            comps[f"termination_{name}_weighted"] = rc[_abi.REWROW_TERM_W + j]
        self.last_reward_components = comps
        st, mk = core.stats, core.masks
        ex = {"consecutive_successes": st[_abi.STAT["CONSECUTIVE_SUCCESSES"]], "episode_length": core.episode_length}
        for i, name in enumerate(_abi.SUCCESS_CRITERIA):
            if (c.active_success_mask >> i) & 1:
                ex[f"success_{name}"] = st[_abi.STAT["SUCC_MEAN"] + i]
                ex[f"success_reason_{name}"] = mk[_abi.MASK_SUCC_REASON + i]
        for i, name in enumerate(_abi.FAILURE_CRITERIA):
            if (c.active_failure_mask >> i) & 1:
                ex[f"failure_{name}"] = st[_abi.STAT["FAIL_MEAN"] + i]
                ex[f"failure_reason_{name}"] = mk[_abi.MASK_FAIL_REASON + i]
        ex["success"], ex["failure"], ex["timeout"] = mk[_abi.MASK_SUCCESS], mk[_abi.MASK_FAILURE], mk[_abi.MASK_TIMEOUT]
        ex["success_rate"] = st[_abi.STAT["SUCCESS_RATE"]]
        ex["failure_rate"] = st[_abi.STAT["FAILURE_RATE"]]
        ex["timeout_rate"] = st[_abi.STAT["TIMEOUT_RATE"]]
        ex["reward_components"] = comps
        self.extras = ex

    # ------------------------------------------------------------------ VecTask properties
    @property
    def num_observations(self):
        if self._num_observations == 0:
            raise RuntimeError("num_observations accessed before initialization.")
        return self._num_observations

    @property
    def num_actions(self):
        if self._num_actions == 0:
            raise RuntimeError("num_actions accessed before initialization.")
        return self._num_actions

    @property
    def observation_space(self):
        return Box(-float("inf"), float("inf"), (self.num_observations,), np.float32)

    @property
    def action_space(self):
        return Box(-1.0, 1.0, (self.num_actions,), np.float32)

    @property
    def episode_time(self):                                      # dexhand_base.py:702-712
        return self.episode_step_count.float() * self.physics_manager.control_dt

    @property
    def random_actions_enabled(self):                            # viewer-only feature, headless => False
        return False

    @property
    def rigid_body_states(self):
        """(N, B, 13), materialised on access (gym.refresh_rigid_body_state_tensor)."""
        self._core.refresh_body_states()
        return self._core.rigid_body_states

    @property
    def contact_forces_all(self):
        self._core.refresh_body_states()
        return self._core.contact_forces_all

    @property
    def contact_forces(self):
        """(N, 5, 3) forces on r_f_link{1..5}_4, the per-step gathered copy (tensor_manager.py:441-446)."""
        return self._core.field("cf5").t().reshape(self.num_envs, 5, 3)

    @property
    def full_dof_targets(self):
        return self._core.full_dof_targets

    # ------------------------------------------------------------------ lifecycle
    def _apply_pre_action_rule(self):
        """The custom pre-action rule (rules.py:78-95).  The reference applies it between compute_observations and
        concatenate_observations (step_processor.py:56-77), i.e. on the obs_dict of the terminal state, before termination,
        rewards and the in-step resets.  Here the fused step has already run all of that with the identity default; nothing
        in termination or rewards reads active_rule_targets, and obs_all still holds the PRE-reset observations, so the
        rule is evaluated afterwards on the same inputs the reference gives it -- obs_dict of the terminal state and the
        pre-reset active_prev_targets (the obs_dict entry, not the post-reset field) -- and its output is patched into
        the field the next action stage reads, the obs_dict row and, when the key is a policy observation, into the
        obs_buf / rollout-sink columns."""
        rule = self.action_processor._pre_action_rule
        if rule is None:       # identity default already written by the post kernel
            return
        if self.obs_dict_mode != "all":
            raise RuntimeError("a custom pre-action rule reads the full obs_dict: create the env with env.obsDict = 'all' (the default)")
        out = rule(self.obs_dict["active_prev_targets"].clone(), {"obs_dict": self.obs_dict, "env": self})
        self._core.field("active_rule_targets").copy_(out.t())
        off, dim = obs_key_offsets()["active_rule_targets"]
        self._core.field("obs_all")[off:off + dim].copy_(out.t())
        sl = self.observation_encoder.component_slice_indices.get("active_rule_targets")
        if sl is not None:
            self.obs_buf[:, sl[0]:sl[1]] = out
            sink = getattr(self._core, "_sink_obs", None)
            if sink is not None:
                sink[:, sl[0]:sl[1]] = out

    def step(self, actions):
        """obs (N,O) f32, rew (N,) f32, done (N,) bool, extras -- views of env-owned buffers."""
        if actions is None:
            raise RuntimeError("Actions cannot be None")
        ap = self.action_processor
        fused = not ap._host_path() and ap._action_rule is None
        if fused and self._actions_copy_bound:
            # DexHandBase.actions = actions.clone() (dexhand_base.py:851): the copy is written by the action block of the
            # step kernel itself (dexsim_set_action_copy) into self.actions -- no clone launch on the hot path
            self._core.step(actions)
            self._apply_pre_action_rule()
            return self.obs_buf, self.rew_buf, self.reset_buf, self.extras
        if self._actions_copy_bound:
            self.actions.copy_(actions)      # keep the tensor the device copy is bound to
        else:
            self.actions = actions.clone()                       # dexhand_base.py:851
        if ap._host_path():
            # custom post-action filter / coupling rule: action stage in torch on the host, then the staged device path
            ap._host_process_actions(self.actions)
            self._core.physics_step(False)
            self._core.post_physics(False)
            self._apply_pre_action_rule()
            return self.obs_buf, self.rew_buf, self.reset_buf, self.extras
        if ap._action_rule is not None:
            config = {"control_mode": ap.action_control_mode, "policy_controls_base": ap.policy_controls_hand_base,
                      "policy_controls_fingers": ap.policy_controls_fingers}
            raw = ap._action_rule(ap.active_prev_targets.clone(), ap.active_rule_targets.clone(), self.actions, config)
            self._core.set_raw_targets(raw)
        self._core.step(self.actions)
        self._apply_pre_action_rule()
        return self.obs_buf, self.rew_buf, self.reset_buf, self.extras

    def reset(self):
        if self.action_processor._pre_action_rule is None:
            self._core.reset()
            return self.obs_buf
        # with a custom pre-action rule the reference's sequence is spelled out, because the rule runs inside BOTH
        # observation passes of reset() (dexhand_base.py:805-838: compute_observations, then post_physics_step)
        core = self._core
        core.begin_step()
        core.reset_idx(torch.arange(self.num_envs, device=self.device))
        core.post_physics(True)
        self._apply_pre_action_rule()
        core.post_physics(False)
        self._apply_pre_action_rule()
        return self.obs_buf

    def reset_idx(self, env_ids):
        if len(env_ids) == 0:
            return
        self._core.reset_idx(env_ids)

    def pre_physics_step(self, actions):
        if self._actions_copy_bound:
            self.actions.copy_(actions)      # keep the tensor the device-side action copy is bound to
        else:
            self.actions = actions.clone()   # dexhand_base.py:851
        self._core.process_actions(self.actions)

    def post_physics_step(self):
        self._core.post_physics(False)
        return self.obs_buf, self.rew_buf, self.reset_buf, self.extras

    def get_observations_dict(self):
        return self.obs_dict.copy()

    def set_rule_based_controllers(self, base_controller=None, finger_controller=None):
        """Rule-based control of the DOF groups the policy does not drive (dexhand_base.py:958-986), realised as a
        pre-action rule that overwrites the uncontrolled part of active_rule_targets."""
        def rule(active_prev_targets, state):
            out = active_prev_targets.clone()
            if base_controller is not None and not self.policy_controls_hand_base:
                out[:, :6] = base_controller(self)
            if finger_controller is not None and not self.policy_controls_fingers:
                out[:, 6:] = finger_controller(self)
            return out
        self.action_processor.set_pre_action_rule(rule if (base_controller or finger_controller) else None)

    # ------------------------------------------------------------------ save / restore / fork (dexsim_save_state and friends)
    def _state_core(self, what):
        core = self._core
        for m in ("state_layout", "state_bank", "save_state", "load_state", "copy_envs", "get_step_stamp", "set_step_stamp"):
            if not hasattr(core, m):
                raise DexSimError(f"{what} needs the HIP engine (DexSimCore): the injected core {type(core).__name__} has no {m}()")
        return core

    def _config_hash(self):
        return hashlib.sha256(bytes(self._sim_cfg) + bytes(self._model_struct)).hexdigest()

    def get_state(self):
        """Full snapshot (EnvState) of this env at a control-step boundary; set_state() of it, here or in a fresh env of the
        same configuration, continues bit for bit."""
        core = self._state_core("get_state")
        bank = core.state_bank(core.NS)
        core.save_state(bank)
        ap = self.action_processor
        return EnvState(bank.version, bank.record_words, self.num_envs, self._config_hash(), bank.capacity, core.get_step_stamp(),
                        bank.data, core.stats.clone(), core.counters.clone(), self.actions.clone(),
                        ap._enabled_post_action_filters)

    def set_state(self, state):
        """Restore a snapshot taken by get_state().  Every env-owned tensor (obs_buf, rew_buf, reset_buf, extras, obs_dict,
        dof_state, actor_root_state_tensor, ...) is written in place: the views callers hold stay valid."""
        core = self._state_core("set_state")
        from .core import StateBank
        layout, words = core.state_layout()
        for name, mine, theirs in (("version", _abi.STATE_VERSION, state.version), ("record_words", words, state.record_words),
                                   ("num_envs", self.num_envs, state.num_envs), ("config_hash", self._config_hash(), state.config_hash)):
            if mine != theirs:
                raise DexSimError(f"set_state: the state does not fit this env: {name} is {theirs}, expected {mine}")
        if state.capacity < core.NS:
            raise DexSimError(f"set_state: the state does not fit this env: capacity is {state.capacity}, expected at least {core.NS}")
        dev = core.device
        bank = StateBank(state.bank.to(dev), state.capacity, state.record_words, layout, state.version)
        core.load_state(bank)
        core.stats.copy_(state.stats.to(dev))
        core.counters.copy_(state.counters.to(dev))
        core.set_step_stamp(state.stamp)
        self.actions.copy_(state.actions.to(self.actions.device))
        self.action_processor._enabled_post_action_filters = list(state.enabled_post_action_filters)

    def state_bank(self, capacity):
        """A state bank of `capacity` slots for save_states / load_states (a bank of grasp states, a curriculum, ...)."""
        return self._state_core("state_bank").state_bank(capacity)

    def save_states(self, bank, slots, env_ids):
        """Records of envs `env_ids` -> slots `slots` of `bank`."""
        self._state_core("save_states").save_state(bank, env_ids=env_ids, slots=slots)

    def load_states(self, bank, slots, env_ids):
        """Slots `slots` of `bank` -> envs `env_ids` (unique): reset-to-stored-state.  Only those envs change."""
        self._state_core("load_states").load_state(bank, env_ids=env_ids, slots=slots)

    def fork_envs(self, src_ids, dst_ids, check=True):
        """Copy env src_ids[i] onto env dst_ids[i] (a source may repeat).  The destinations must be unique and none may also be a
        source; check=True verifies that (and the id range) on the device, which costs a host synchronisation: pass
        check=False when forking every step with ids known to be good."""
        core = self._state_core("fork_envs")
        src = torch.as_tensor(src_ids, device=core.device).to(torch.int64).view(-1)
        dst = torch.as_tensor(dst_ids, device=core.device).to(torch.int64).view(-1)
        if src.numel() != dst.numel():
            raise DexSimError(f"fork_envs: {src.numel()} sources but {dst.numel()} destinations")
        if check and src.numel():
            n = self.num_envs
            hits = torch.zeros(n, dtype=torch.int32, device=core.device)
            ok = bool(((src >= 0) & (src < n)).all() & ((dst >= 0) & (dst < n)).all())
            if not ok:
                raise DexSimError(f"fork_envs: env ids must be in [0, {n})")
            hits.index_add_(0, dst, torch.ones_like(dst, dtype=torch.int32))
            is_src = torch.zeros(n, dtype=torch.bool, device=core.device)
            is_src[src] = True
            if bool((hits > 1).any()):
                raise DexSimError("fork_envs: a destination env is listed more than once")
            if bool(((hits > 0) & is_src).any()):
                raise DexSimError("fork_envs: a destination env is also a source")
        core.copy_envs(src, dst)

    # ------------------------------------------------------------------ camera sensors (dexsim_render)
    def _render_core(self, what):
        core = self._core
        if not hasattr(core, "render"):
            raise NotImplementedError(f"{what} needs the HIP engine (DexSimCore): the injected core {type(core).__name__} has no render()")
        return core

    def _camera(self, name):
        if name not in self._cameras:
            raise KeyError(f"no camera named '{name}' (cameras: {sorted(self._cameras)})")
        return self._cameras[name]

    def create_camera(self, name, width, height, hfov_deg=75.0, eye=(-1.5, 0.0, 0.5), target=(0.0, 0.0, 0.15), parent=None,
                      near=0.01, far=10.0):
        """A camera sensor for every env (GraphicsManager.create_camera, graphics_manager.py:56-100).  eye / target: the look-at
        pair in the parent frame, shared 3-vectors or (N, 3) tensors; parent: None = each env's world frame, or a joint index /
        DOF name to mount the camera on that joint's frame (e.g. 5 or "ARRz": eye-in-hand on the palm joint), up = the parent's +z.
        near / far: clip distances along the optical axis in metres."""
        core = self._render_core("create_camera")
        if name in self._cameras:
            raise ValueError(f"camera '{name}' already exists")
        if parent is None:
            pj = -1
        elif isinstance(parent, str):
            if parent not in self.model.dof_names:
                raise ValueError(f"create_camera: unknown joint '{parent}' (joints: {self.model.dof_names})")
            pj = self.model.dof_names.index(parent)
        else:
            pj = int(parent)
        if not -1 <= pj < _abi.NJ:
            raise ValueError(f"create_camera: parent joint index must be in [0, {_abi.NJ}), got {parent}")
        width, height = int(width), int(height)
        if not (1 <= width <= _abi.RENDER_MAX_DIM and 1 <= height <= _abi.RENDER_MAX_DIM):
            raise ValueError(f"create_camera: width and height must be in [1, {_abi.RENDER_MAX_DIM}], got {width} x {height}")
        if not 0.0 < float(hfov_deg) < 180.0:
            raise ValueError(f"create_camera: hfov_deg must be in (0, 180), got {hfov_deg}")
        if not float(near) < float(far):
            raise ValueError(f"create_camera: near ({near}) must be below far ({far})")
        cam = _abi.DexSimCamera()
        cam.width, cam.height, cam.hfov_deg = width, height, float(hfov_deg)
        cam.near_clip, cam.far_clip, cam.parent_joint = float(near), float(far), pj
        core.render_layout()
        self._cameras[name] = {"cam": cam, "eye": None, "target": None, "buffers": {}}
        self.set_camera_location(name, eye, target)
        return name

    def set_camera_location(self, name, eye, target):
        """GraphicsManager.set_camera_location (graphics_manager.py:102-134): eye and target in the camera's parent frame, each a
        shared 3-vector or an (N, 3) tensor with one row per env."""
        c = self._camera(name)
        for key, val in (("eye", eye), ("target", target)):
            t = torch.as_tensor(val, dtype=torch.float32)
            if tuple(t.shape) == (3,):
                for i in range(3):
                    getattr(c["cam"], key)[i] = float(t[i])
                c[key] = None
            elif tuple(t.shape) == (self.num_envs, 3):
                c[key] = t.to(self._core.device).contiguous()
            else:
                raise ValueError(f"set_camera_location: {key} must have shape (3,) or ({self.num_envs}, 3), got {tuple(t.shape)}")

    def render_camera(self, name, env_ids=None, outputs=("rgba", "depth", "seg")):
        """GraphicsManager.render_all_cameras + capture_frame (graphics_manager.py:136-179) for one camera: a dict of device
        tensors -- "rgba" (k, H, W, 4) uint8, "depth" (k, H, W) float32 (+inf without a hit), "seg" (k, H, W) int32 -- for the
        envs `env_ids` (None = all, k = num_envs).  The tensors belong to the camera: they are allocated once per k and
        overwritten by the next render_camera of the same camera and k."""
        core = self._render_core("render_camera")
        c = self._camera(name)
        outputs = tuple(outputs)
        if not outputs or any(o not in ("rgba", "depth", "seg") for o in outputs):
            raise ValueError(f"render_camera: outputs must be a non-empty subset of ('rgba', 'depth', 'seg'), got {outputs}")
        ids = None if env_ids is None else torch.as_tensor(env_ids, device=core.device).to(torch.int64).view(-1)
        k = self.num_envs if ids is None else int(ids.numel())
        cam, dev = c["cam"], core.device
        H, W = int(cam.height), int(cam.width)
        buf = c["buffers"].setdefault(k, {})
        if "scene" not in buf:
            buf["scene"] = torch.zeros(k, core.render_layout()[1], dtype=torch.float32, device=dev)
        shapes = {"rgba": ((k, H, W, 4), torch.uint8), "depth": ((k, H, W), torch.float32), "seg": ((k, H, W), torch.int32)}
        for o in outputs:
            if o not in buf:
                buf[o] = torch.zeros(shapes[o][0], dtype=shapes[o][1], device=dev)
        if k == 0:
            return {o: buf[o] for o in outputs}
        pick = lambda t: None if t is None else (t if ids is None else t[ids].contiguous())
        core.render(cam, buf["scene"], env_ids=ids, eye=pick(c["eye"]), target=pick(c["target"]),
                    **{o: buf[o] for o in outputs})
        return {o: buf[o] for o in outputs}

    def render(self, mode="rgb_array"):
        """env 0's (H, W, 3) uint8 frame of the camera named "video" (created by a video_config with a `resolution`, or by
        create_camera("video", ...)); None without one -- headless: no viewer / recorder / streamer."""
        if "video" not in getattr(self, "_cameras", {}):
            return None
        return self.render_camera("video", [0], ("rgba",))["rgba"][0, :, :, :3].cpu().numpy()

    # ------------------------------------------------------------------ Jacobians, mass matrix, gravity force
    def _kindyn_rows(self, what, method, env_ids, q):
        """The HIP core (it must have `method`), (ids, q) as device tensors and the number of output rows k, for the queries
        that are functions of q: get_jacobian, get_mass_matrix, solve_fingertip_ik, query_proximity."""
        core = self._core
        if not hasattr(core, method):
            raise NotImplementedError(f"{what} needs the HIP engine (DexSimCore): the injected core {type(core).__name__} has no {method}()")
        if q is not None:
            q = torch.as_tensor(q, dtype=torch.float32, device=core.device)
            if q.dim() != 2 or q.shape[1] != _abi.NJ or q.shape[0] < 1:
                raise ValueError(f"{what}: q must have shape (k, {_abi.NJ}) with k >= 1, got {tuple(q.shape)}")
            return core, None, q.contiguous(), int(q.shape[0])
        if env_ids is None:
            return core, None, None, self.num_envs
        ids = torch.as_tensor(env_ids, device=core.device).to(torch.int64).view(-1)
        if ids.numel() < 1:
            raise ValueError(f"{what}: env_ids is empty")
        return core, ids, None, int(ids.numel())

    def _kindyn_out(self, what, out, shape, device):
        if out is None:
            return torch.empty(shape, dtype=torch.float32, device=device)      # the kernels write every element
        if not torch.is_tensor(out) or tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() \
                or out.device != device:
            raise ValueError(f"{what}: out must be a contiguous float32 tensor of shape {shape} on {device}")
        return out

    def _kindyn_bodies(self, what, bodies):
        """(indices or None = all, nb) of a `bodies` argument: indices into the rows of rigid_body_states or names from
        hand_model.BODY_NAMES."""
        if bodies is None:
            return None, _abi.NUM_HAND_BODIES
        if isinstance(bodies, (str, int)):
            bodies = [bodies]
        idx = []
        for b in bodies:
            if isinstance(b, str):
                if b not in self.model.body_names:
                    raise ValueError(f"{what}: unknown body '{b}' (bodies: {self.model.body_names})")
                b = self.model.body_names.index(b)
            b = int(b)
            if not 0 <= b < _abi.NUM_HAND_BODIES:
                raise ValueError(f"{what}: body index must be in [0, {_abi.NUM_HAND_BODIES}), got {b}")
            idx.append(b)
        if not 1 <= len(idx) <= _abi.NUM_HAND_BODIES:
            raise ValueError(f"{what}: between 1 and {_abi.NUM_HAND_BODIES} bodies, got {len(idx)}")
        return idx, len(idx)

    def get_jacobian(self, bodies=None, env_ids=None, q=None, out=None):
        """gym.acquire_jacobian_tensor / refresh_jacobian_tensors for the hand: (k, nb, 6, 26) geometric Jacobians of the hand
        bodies `bodies` -- indices into the rows of rigid_body_states or names from hand_model.BODY_NAMES such as
        "r_f_link2_tip"; None = all 37 in order.  Rows 0-2: world linear velocity of the body origin, 3-5: world angular
        velocity; column j: DOF j of dof_state, so jac[i, b] @ dof_vel[env] == rigid_body_states[env, b, 7:13].  Rows: the
        envs `env_ids` (None = all), or the rows of a (k, 26) joint-position override `q` (env_ids is then ignored)."""
        core, ids, q, k = self._kindyn_rows("get_jacobian", "body_jacobian", env_ids, q)
        idx, nb = self._kindyn_bodies("get_jacobian", bodies)
        out = self._kindyn_out("get_jacobian", out, (k, nb, 6, _abi.NJ), core.device)
        core.body_jacobian(out, env_ids=ids, q=q, bodies=idx)
        return out

    def get_mass_matrix(self, env_ids=None, q=None, gravity=False, out=None):
        """gym.acquire_mass_matrix_tensor / refresh_mass_matrix_tensors for the hand: the (k, 26, 26) joint-space inertia M(q)
        (no armature, no PD terms).  gravity=True returns (M, g) with g (k, 26) the gravity force dV/dq: the generalized force
        a controller adds to hold the hand.  Rows as for get_jacobian.  out: M, or the pair (M, g) when gravity=True."""
        core, ids, q, k = self._kindyn_rows("get_mass_matrix", "mass_matrix", env_ids, q)
        if gravity:
            if out is not None and (not isinstance(out, (tuple, list)) or len(out) != 2):
                raise ValueError("get_mass_matrix: with gravity=True, out must be the pair (M, g)")
            om, og = (None, None) if out is None else out
            M = self._kindyn_out("get_mass_matrix", om, (k, _abi.NJ, _abi.NJ), core.device)
            g = self._kindyn_out("get_mass_matrix", og, (k, _abi.NJ), core.device)
            core.mass_matrix(mass=M, gravity=g, env_ids=ids, q=q)
            return M, g
        M = self._kindyn_out("get_mass_matrix", out, (k, _abi.NJ, _abi.NJ), core.device)
        core.mass_matrix(mass=M, env_ids=ids, q=q)
        return M

    # ------------------------------------------------------------------ inverse dynamics, bias accelerations
    def _kindyn_rows_qd(self, what, method, env_ids, q, qd):
        """_kindyn_rows for the queries that are functions of (q, qd): the overrides go together."""
        core, ids, qt, k = self._kindyn_rows(what, method, env_ids, q)
        if (q is None) != (qd is None):
            raise ValueError(f"{what}: q and qd go together: both None (the envs' state) or both (k, {_abi.NJ}) overrides")
        return core, ids, qt, self._kindyn_vel(what, "qd", qd, k, core.device), k

    def _kindyn_vel(self, what, name, t, k, device):
        if t is None:
            return None
        t = torch.as_tensor(t, dtype=torch.float32, device=device)
        if tuple(t.shape) != (k, _abi.NJ):
            raise ValueError(f"{what}: {name} must have shape ({k}, {_abi.NJ}), got {tuple(t.shape)}")
        return t.contiguous()

    def get_inverse_dynamics(self, qdd=None, env_ids=None, q=None, qd=None, gravity=True, out=None):
        """(k, 26) generalized forces tau = M(q) qdd + c(q, qd) (+ g(q) with gravity=True) that produce the joint accelerations
        `qdd` (k, 26; None = zero), with the M and g of get_mass_matrix: no armature, no PD terms, no contact.  Rows: the envs
        `env_ids` (None = all) at their dof_pos / dof_vel, or the rows of the (k, 26) overrides `q` and `qd`, which go together
        (env_ids is then ignored).  Row i of qdd belongs to row i of the result on either path."""
        core, ids, q, qd, k = self._kindyn_rows_qd("get_inverse_dynamics", "inverse_dynamics", env_ids, q, qd)
        qdd = self._kindyn_vel("get_inverse_dynamics", "qdd", qdd, k, core.device)
        out = self._kindyn_out("get_inverse_dynamics", out, (k, _abi.NJ), core.device)
        core.inverse_dynamics(out, qdd=qdd, env_ids=ids, q=q, qd=qd, gravity=gravity)
        return out

    def get_bias_forces(self, env_ids=None, q=None, qd=None, gravity=True, out=None):
        """get_inverse_dynamics at qdd = 0: the (k, 26) velocity-product force c(q, qd), plus g(q) with gravity=True -- what a
        computed-torque controller adds to M(q) qdd."""
        return self.get_inverse_dynamics(None, env_ids, q, qd, gravity, out)

    def get_body_bias_acceleration(self, bodies=None, env_ids=None, q=None, qd=None, out=None):
        """(k, nb, 6) Jdot qd of the hand bodies `bodies` (as for get_jacobian): world linear acceleration of the body origin
        (0-2) and angular acceleration (3-5) at zero joint acceleration, without gravity, so that get_jacobian(...)[i, b] @ qdd +
        this is the derivative of rigid_body_states[env, b, 7:13].  Rows as for get_inverse_dynamics."""
        core, ids, q, qd, k = self._kindyn_rows_qd("get_body_bias_acceleration", "body_bias_accel", env_ids, q, qd)
        idx, nb = self._kindyn_bodies("get_body_bias_acceleration", bodies)
        out = self._kindyn_out("get_body_bias_acceleration", out, (k, nb, 6), core.device)
        core.body_bias_accel(out, env_ids=ids, q=q, qd=qd, bodies=idx)
        return out

    # ------------------------------------------------------------------ forward dynamics, mass-matrix solves
    def get_forward_dynamics(self, tau=None, env_ids=None, q=None, qd=None, gravity=True, armature=False, out=None):
        """(k, 26) joint accelerations qdd = (M(q) [+ A])^-1 (tau - c(q, qd) [- g(q)]) that the generalized forces `tau` (k, 26;
        None = zero: the free acceleration) produce -- the inverse of get_inverse_dynamics, with the same M, c and g: no PD terms,
        no contact, no joint-limit forces (fold them into tau).  armature=True solves with M + diag(model.armature).  Rows as for
        get_inverse_dynamics; row i of tau belongs to row i of the result on either path."""
        core, ids, q, qd, k = self._kindyn_rows_qd("get_forward_dynamics", "forward_dynamics", env_ids, q, qd)
        tau = self._kindyn_vel("get_forward_dynamics", "tau", tau, k, core.device)
        out = self._kindyn_out("get_forward_dynamics", out, (k, _abi.NJ), core.device)
        core.forward_dynamics(out, tau=tau, env_ids=ids, q=q, qd=qd, gravity=gravity, armature=armature)
        return out

    def solve_mass_matrix(self, rhs, env_ids=None, q=None, armature=False, out=None):
        """(M(q) [+ A])^-1 applied to `rhs` (k, 26) or (k, nrhs, 26), nrhs <= 32, without forming M; the result has rhs's shape.
        Each row is factored once for all its right-hand sides.  With rows of get_jacobian as right-hand sides this is
        M^-1 J^T (Lambda^-1 = J M^-1 J^T), with 26 unit columns M^-1 itself.  Rows as for get_mass_matrix; `out` may be `rhs`."""
        core, ids, q, k = self._kindyn_rows("solve_mass_matrix", "mass_solve", env_ids, q)
        rhs = torch.as_tensor(rhs, dtype=torch.float32, device=core.device)
        if rhs.dim() not in (2, 3) or rhs.shape[0] != k or rhs.shape[-1] != _abi.NJ or \
                (rhs.dim() == 3 and not 1 <= rhs.shape[1] <= _abi.MSOLVE_MAX_RHS):
            raise ValueError(f"solve_mass_matrix: rhs must have shape ({k}, {_abi.NJ}) or ({k}, nrhs, {_abi.NJ}) with nrhs in "
                             f"[1, {_abi.MSOLVE_MAX_RHS}], got {tuple(rhs.shape)}")
        shape = tuple(rhs.shape)
        out = self._kindyn_out("solve_mass_matrix", out, shape, core.device)
        core.mass_solve(out.view(k, -1, _abi.NJ), rhs.contiguous().view(k, -1, _abi.NJ), env_ids=ids, q=q, armature=armature)
        return out

    # ------------------------------------------------------------------ derivatives of the inverse and the forward dynamics
    def _kindyn_outs(self, what, out, shapes, device):
        """_kindyn_out for a call with several outputs: `out` is None or a tuple / list with one tensor per shape."""
        if out is not None and (not isinstance(out, (tuple, list)) or len(out) != len(shapes)):
            raise ValueError(f"{what}: out must be a tuple of {len(shapes)} tensors")
        return [self._kindyn_out(what, o, s, device) for o, s in zip(out or [None] * len(shapes), shapes)]

    def get_inverse_dynamics_derivatives(self, qdd=None, env_ids=None, q=None, qd=None, gravity=True, out=None):
        """(dtau_dq, dtau_dqd), each (k, 26, 26): the derivatives of get_inverse_dynamics(qdd, ...) with respect to the joint
        positions and velocities at fixed qdd, analytic.  D[i, r, c] = d tau_r / d q_c, so D[i] @ dq is the first-order change of
        tau.  The two are TRANSPOSED VIEWS of the device's derivative-major arrays (dexsim.h): call .contiguous() for a dense
        matrix, or .transpose(1, 2) for the (k, c, r) array as it was written.  Arguments and rows as for get_inverse_dynamics.
        out: a pair of contiguous (k, 26, 26) tensors that receive the derivative-major arrays; the views returned are of them."""
        what = "get_inverse_dynamics_derivatives"
        core, ids, q, qd, k = self._kindyn_rows_qd(what, "inverse_dynamics_derivatives", env_ids, q, qd)
        qdd = self._kindyn_vel(what, "qdd", qdd, k, core.device)
        dq, dqd = self._kindyn_outs(what, out, [(k, _abi.NJ, _abi.NJ)] * 2, core.device)
        core.inverse_dynamics_derivatives(dq, dqd, qdd=qdd, env_ids=ids, q=q, qd=qd, gravity=gravity)
        return dq.transpose(1, 2), dqd.transpose(1, 2)

    def get_forward_dynamics_derivatives(self, tau=None, env_ids=None, q=None, qd=None, gravity=True, armature=False, out=None):
        """(qdd, dqdd_dq, dqdd_dqd): the (k, 26) result of get_forward_dynamics(tau, ...) and its (k, 26, 26) derivatives with
        respect to the joint positions and velocities at fixed tau, D[i, r, c] = d qdd_r / d q_c, as transposed views like
        get_inverse_dynamics_derivatives.  d qdd / d tau is (M [+ A])^-1: solve_mass_matrix of 26 unit columns.  Unbounded at
        the base's gimbal lock, where M is singular.  Arguments and rows as for get_forward_dynamics.  out: a triple of contiguous
        tensors (k, 26), (k, 26, 26), (k, 26, 26) that receive qdd and the derivative-major arrays."""
        what = "get_forward_dynamics_derivatives"
        core, ids, q, qd, k = self._kindyn_rows_qd(what, "forward_dynamics_derivatives", env_ids, q, qd)
        tau = self._kindyn_vel(what, "tau", tau, k, core.device)
        qdd, dq, dqd = self._kindyn_outs(what, out, [(k, _abi.NJ)] + [(k, _abi.NJ, _abi.NJ)] * 2, core.device)
        core.forward_dynamics_derivatives(qdd, dq, dqd, tau=tau, env_ids=ids, q=q, qd=qd, gravity=gravity, armature=armature)
        return qdd, dq.transpose(1, 2), dqd.transpose(1, 2)

    # ------------------------------------------------------------------ fingertip inverse kinematics
    @property
    def control_names(self):
        """Names of the 18 active targets in their order: the six base joints, then the first DOF of each finger control's
        coupling group (FINGER_COUPLING_MAP)."""
        return list(self.model.dof_names[:6]) + [FINGER_COUPLING_MAP[c][0][0] for c in range(12)]

    def solve_fingertip_ik(self, targets, env_ids=None, q=None, sites="tips", frame="world", free="fingers", weights=None,
                           iters=16, damping=1e-3, max_step=0.5, return_info=False):
        """Batched inverse kinematics for the five fingertips in control space, every iteration inside one kernel launch.
        targets (k, 5, 3): wanted positions of the fingertip sites (sites="tips") or fingerpad sites (sites="pads"), thumb to
        pinky, in the env's world frame (frame="world", as obs_dict["fingertip_poses_world"][..., :3]) or in the hand frame
        (frame="hand", as fingertip_poses_hand / fingerpad_poses_hand; the base is then fixed).  Rows as for get_jacobian: the
        envs `env_ids` (None = all) start from their current joint positions, the rows of a (k, 26) override `q` from that.
        free: the controls that may move -- "fingers" (controls 6..17), "all", or a list of indices / names (control_names, or
        the hardware names "th_rot", "ff_spr", ...); the others keep their start value.  weights: five values >= 0, 0 drops a
        finger from the objective (a thumb-index pinch: (1, 1, 0, 0, 0)).  Damped least squares with damping `damping`; no
        control changes by more than `max_step` per iteration; the result respects the active limits.  Base slides (m) and base
        rotations (rad) share the one damping.

        Returns controls (k, 18): the 18 active targets the action stage works in.  Feed them back as the raw targets of a
        custom action rule -- env.action_processor.set_action_rule(lambda prev, rule, actions, cfg: controls) -- or, for a
        policy-style action in position mode, through the limit scaling: action = 2 (u - lower) / (upper - lower) - 1 on the
        controls the policy drives.  With return_info=True: (controls, {"q": (k, 26) coupled joint positions, "residual": (k, 5)
        distance left per finger, dropped fingers included})."""
        what = "solve_fingertip_ik"
        core, ids, q, k = self._kindyn_rows(what, "solve_ik", env_ids, q)
        if sites not in ("tips", "pads"):
            raise ValueError(f"{what}: sites must be 'tips' or 'pads', got {sites!r}")
        if frame not in ("world", "hand"):
            raise ValueError(f"{what}: frame must be 'world' or 'hand', got {frame!r}")
        names = self.control_names
        hw = {n: names.index(dofs[0]) for n, dofs in HARDWARE_MAPPING}
        if isinstance(free, str) and free in ("fingers", "all"):
            idx = list(range(6, _abi.NACT)) if free == "fingers" else list(range(_abi.NACT))
        else:
            if isinstance(free, (str, int)):
                free = [free]
            idx = []
            for c in free:
                if isinstance(c, str):
                    if c not in names and c not in hw:
                        raise ValueError(f"{what}: free: unknown control '{c}' (controls: {names}, or {sorted(hw)})")
                    c = names.index(c) if c in names else hw[c]
                c = int(c)
                if not 0 <= c < _abi.NACT:
                    raise ValueError(f"{what}: free: control index must be in [0, {_abi.NACT}), got {c}")
                idx.append(c)
            if not idx:
                raise ValueError(f"{what}: free: at least one control must be free")
        mask = 0
        for c in idx:
            mask |= 1 << c
        if frame == "hand" and mask & 63:
            raise ValueError(f"{what}: free: hand-frame targets need the base controls 0..5 fixed")
        w = [1.0] * _abi.NFINGER if weights is None else [float(x) for x in torch.as_tensor(weights, dtype=torch.float32).view(-1).tolist()]
        if len(w) != _abi.NFINGER or not all(x >= 0.0 and x == x and x != float("inf") for x in w) or not any(x > 0.0 for x in w):
            raise ValueError(f"{what}: weights must be {_abi.NFINGER} finite values >= 0, not all 0, got {w}")
        iters = int(iters)
        if not 1 <= iters <= _abi.IK_MAX_ITERS:
            raise ValueError(f"{what}: iters must be in [1, {_abi.IK_MAX_ITERS}], got {iters}")
        if not float(damping) > 0.0 or not float(max_step) > 0.0:
            raise ValueError(f"{what}: damping and max_step must be positive, got {damping} and {max_step}")
        targets = torch.as_tensor(targets, dtype=torch.float32, device=core.device)
        if tuple(targets.shape) != (k, _abi.NFINGER, 3):
            raise ValueError(f"{what}: targets must have shape ({k}, {_abi.NFINGER}, 3), got {tuple(targets.shape)}")
        controls = torch.empty((k, _abi.NACT), dtype=torch.float32, device=core.device)
        info = {}
        if return_info:
            info = {"q": torch.empty((k, _abi.NJ), dtype=torch.float32, device=core.device),
                    "residual": torch.empty((k, _abi.NFINGER), dtype=torch.float32, device=core.device)}
        if ids is not None:   # a row whose id is out of range is left as it is by the kernel: give it a defined value
            controls.fill_(float("nan"))
            for t in info.values():
                t.fill_(float("nan"))
        core.solve_ik(targets.contiguous(), controls, env_ids=ids, q=q, sites=0 if sites == "tips" else 1,
                      frame=0 if frame == "world" else 1, free_mask=mask, weights=w, iters=iters, damping=float(damping),
                      max_step=float(max_step), q_out=info.get("q"), residual=info.get("residual"))
        return (controls, info) if return_info else controls

    # ------------------------------------------------------------------ clearance queries (dexsim_query_proximity)
    def query_proximity(self, env_ids=None, q=None, box_pose=None, box_size=None, outputs=("cap_env", "self_min", "pair_dist"), out=None):
        """Clearances of the hand against the box, the ground and itself, one kernel launch: is a configuration free of collision,
        and how far is every link from the object, the ground and the other fingers?  Returns a ProximityResult with
          cap_env   (k, 18, 2, 8): per collision capsule, record 0 against the box and record 1 against the ground z = 0 --
                    [signed distance, unit normal towards the capsule (3), witness point on the other shape (3), axis parameter t];
                    without a box the box record is (+inf, 0, ...)
          self_min  (k, 15, 8): the closest capsule pair of the ten finger pairs and of the palm with each finger --
                    [distance, normal from B to A (3), witness on B's surface (3), pair index as int32 bits]
          pair_dist (k, 120): the distance of every pair of `pairs`, the (120, 3) table (capsule A, capsule B, group)
        (the tensors not named in `outputs` are None).  Rows as for get_jacobian: the envs `env_ids` (None = all), or the rows of a
        (k, 26) joint-position override `q`.  The box: `box_pose` (k, 7) = centre xyz + quaternion xyzw when given; "env" together
        with a `q` of num_envs rows takes every env's own box ("check my IK result against my box"); None = the envs' own box
        without `q`, no box with it.  box_size: edge length, None = the configured one.  out: a dict of preallocated tensors by
        output name.  The engine's own hand self-collision does not exist: negative self distances are not resolved by the
        physics."""
        what = "query_proximity"
        core, ids, q, k = self._kindyn_rows(what, "proximity", env_ids, q)
        names = ("cap_env", "self_min", "pair_dist")
        if isinstance(outputs, str):
            outputs = (outputs,)
        outputs = tuple(outputs)
        if not outputs or any(o not in names for o in outputs):
            raise ValueError(f"{what}: outputs must be a non-empty subset of {names}, got {outputs}")
        if isinstance(box_pose, str):
            if box_pose != "env":
                raise ValueError(f"{what}: box_pose must be a (k, 7) tensor, 'env' or None, got {box_pose!r}")
            if q is None or k != self.num_envs:
                raise ValueError(f"{what}: box_pose='env' needs a q override of num_envs = {self.num_envs} rows")
            if not int(self._sim_cfg.has_box):
                raise ValueError(f"{what}: box_pose='env' needs a task with a box")
            box_pose = core.root_state[:, 1, :7].contiguous()
        elif box_pose is not None:
            box_pose = torch.as_tensor(box_pose, dtype=torch.float32, device=core.device)
            if tuple(box_pose.shape) != (k, 7):
                raise ValueError(f"{what}: box_pose must have shape ({k}, 7), got {tuple(box_pose.shape)}")
            box_pose = box_pose.contiguous()
        size = 0.0
        if box_size is not None:
            size = float(box_size)
            if not (size > 0.0 and size != float("inf")):
                raise ValueError(f"{what}: box_size must be a positive finite edge length, got {box_size}")
        shapes = {"cap_env": (k, _abi.NCAP, 2, 8), "self_min": (k, _abi.NPROX_GROUPS, 8), "pair_dist": (k, _abi.NPROX_PAIRS)}
        if out is not None and (not isinstance(out, dict) or any(o not in outputs for o in out)):
            raise ValueError(f"{what}: out must be a dict of tensors keyed by the names in outputs, got {out if not isinstance(out, dict) else sorted(out)}")
        bufs = {}
        for o in outputs:
            given = None if out is None else out.get(o)
            bufs[o] = self._kindyn_out(what, given, shapes[o], core.device)
            if given is None and ids is not None:   # a row whose id is out of range is left as it is by the kernel: give it a defined value
                bufs[o].fill_(float("nan"))
        core.proximity(env_ids=ids, q=q, box_pose=box_pose, box_size=size, **bufs)
        if getattr(self, "_proximity_pairs", None) is None:
            self._proximity_pairs = core.proximity_pairs()                     # a host table: read once
        return ProximityResult(self.model, self._proximity_pairs, **bufs)

    def close(self):
        if self._core is not None:
            self._core.close()

    # rl_games-side expectations (rl/__init__.py:39-59)
    def get_env_info(self):
        return {"action_space": self.action_space, "observation_space": self.observation_space, "num_envs": self.num_envs}

    def get_number_of_agents(self):
        return 1
