"""DexSimCore: device memory + streams plumbing around the C-ABI (PyTorch-ROCm is used only for allocation,
the current stream and tensor views; every computation is a HIP kernel launched by libdexsim)."""
import ctypes as C

import torch

from . import _abi
from ._lib import DexSimError, check, load


class StateBank:
    """A caller-owned state bank (include/dexsim.h): `data` is the flat float32 device tensor the library reads and writes,
    the rest is what has to stay with it -- capacity, the record size and DEXSIM_STATE_VERSION."""

    def __init__(self, data, capacity, record_words, layout, version=_abi.STATE_VERSION):
        self.data, self.capacity, self.record_words, self.version = data, int(capacity), int(record_words), int(version)
        self.layout = layout                      # name -> (word offset in the record, rows, is_int)
        self.stride = (self.capacity + 63) // 64 * 64

    def section(self, name):
        """(rows, capacity) view of one section of the records, float32 or int32.  wlam is stored [quad][slot][4]: its view
        is permuted so that row 4 q + c is word c of quad q, like every other section."""
        off, rows, is_int = self.layout[name]
        base = self.data.view(torch.int32) if is_int else self.data
        flat = base[off * self.stride: (off + rows) * self.stride]
        if name == "wlam":
            return flat.view(rows // 4, self.stride, 4).permute(0, 2, 1).reshape(rows, self.stride)[:, : self.capacity]
        return flat.view(rows, self.stride)[:, : self.capacity]


class DexSimCore:
    def __init__(self, sim_cfg, model_struct, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise DexSimError(f"dexsim needs a HIP device (got '{device}'): there is no CPU backend")
        if not torch.cuda.is_available():
            raise DexSimError("no HIP device visible to PyTorch-ROCm")
        self.lib = load()
        self.cfg = sim_cfg
        self.model = model_struct
        self.device = device
        self.N = int(sim_cfg.num_envs)
        self.NS = (self.N + 63) // 64 * 64
        dev_index = device.index if device.index is not None else torch.cuda.current_device()
        self.dev_index = dev_index

        fields = (_abi.DexSimField * 128)()
        nf, words = C.c_int(0), C.c_size_t(0)
        check(self.lib.dexsim_arena_layout(C.byref(sim_cfg), fields, 128, C.byref(nf), C.byref(words)), "arena_layout")
        self.arena = torch.zeros(words.value, dtype=torch.float32, device=device)
        self._arena_i32 = self.arena.view(torch.int32)
        self.fields = {}
        for i in range(nf.value):
            f = fields[i]
            self.fields[f.name.decode()] = (int(f.offset), int(f.rows), bool(f.is_int))

        N = self.N
        A = 1 + int(sim_cfg.has_box)
        B = _abi.NUM_HAND_BODIES + int(sim_cfg.has_box)
        self.num_bodies, self.num_actors = B, A
        z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=device)
        self.stats = z(_abi.STAT_WORDS)
        self.counters = z(_abi.STAT_WORDS, dtype=torch.int32)
        self.obs_buf = z(N, sim_cfg.num_obs)
        self.rew_buf = z(N)
        self.reset_buf = z(N, dtype=torch.bool)
        self.episode_step_count = z(N, dtype=torch.int64)
        self.episode_length = z(N, dtype=torch.int64)
        self.dof_state = z(N, _abi.NJ, 2)
        self.root_state = z(N, A, 13)
        self.rigid_body_states = z(N, B, 13)
        self.contact_forces_all = z(N, B, 3)
        self.full_dof_targets = z(N, _abi.NJ)
        self.reset_samples = None
        self.masks = z(_abi.NUM_MASKS, N, dtype=torch.bool)
        self.raw_targets = None

        self.h = C.c_void_p()
        check(self.lib.dexsim_create(C.byref(sim_cfg), C.byref(model_struct), dev_index, C.byref(self.h)), "create")
        self._bind()
        self.init_state()

    # ------------------------------------------------------------------ plumbing
    def _bind(self):
        b = _abi.DexSimBuffers()
        b.arena = self.arena.data_ptr()
        b.stats, b.counters = self.stats.data_ptr(), self.counters.data_ptr()
        b.obs_buf, b.rew_buf, b.reset_buf = self.obs_buf.data_ptr(), self.rew_buf.data_ptr(), self.reset_buf.data_ptr()
        b.episode_step_count, b.episode_length = self.episode_step_count.data_ptr(), self.episode_length.data_ptr()
        b.dof_state, b.root_state = self.dof_state.data_ptr(), self.root_state.data_ptr()
        b.rigid_body_states, b.contact_forces_all = self.rigid_body_states.data_ptr(), self.contact_forces_all.data_ptr()
        b.full_dof_targets = self.full_dof_targets.data_ptr()
        b.reset_samples = self.reset_samples.data_ptr() if self.reset_samples is not None else None
        b.masks = self.masks.data_ptr()
        b.raw_targets = self.raw_targets.data_ptr() if self.raw_targets is not None else None
        check(self.lib.dexsim_bind(self.h, C.byref(b)), "bind")

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.lib.dexsim_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def field(self, name):
        """(rows, N) view of an arena field (float32 or int32); padded lanes are sliced off."""
        off, rows, is_int = self.fields[name]
        base = self._arena_i32 if is_int else self.arena
        return base[off: off + rows * self.NS].view(rows, self.NS)[:, : self.N]

    def set_reset_samples(self, samples):
        """Inject the 29 uniforms/env of the next resets (parity tests); None -> device Philox stream."""
        if samples is None:
            self.reset_samples = None
        else:
            s = torch.as_tensor(samples, dtype=torch.float32, device=self.device).contiguous()
            assert s.shape == (self.N, _abi.NRESET_SAMPLES)
            self.reset_samples = s
        self._bind()

    def set_raw_targets(self, raw):
        """(N, 18) output of a host-side custom action rule for the next process_actions; None -> built-in rule."""
        if raw is None:
            if self.raw_targets is not None:
                self.raw_targets = None
                self._bind()
            return
        first = self.raw_targets is None
        if first:
            self.raw_targets = torch.zeros(self.N, _abi.NACT, device=self.device)
        self.raw_targets.copy_(raw)
        if first:
            self._bind()

    def _actions_ptr(self, actions):
        if actions is None:
            raise RuntimeError("Actions cannot be None")
        if actions.device != self.device or actions.dtype != torch.float32 or not actions.is_contiguous():
            actions = actions.to(device=self.device, dtype=torch.float32).contiguous()
        if tuple(actions.shape) != (self.N, int(self.cfg.num_actions)):
            raise DexSimError(f"actions must have shape ({self.N}, {int(self.cfg.num_actions)}), got {tuple(actions.shape)}")
        self._keep = actions  # keep alive until the kernel ran
        return C.c_void_p(actions.data_ptr())

    def _ids_ptr(self, env_ids):
        ids = torch.as_tensor(env_ids, device=self.device).to(torch.int64).contiguous()
        self._keep_ids = ids
        return C.c_void_p(ids.data_ptr()), int(ids.numel())

    # ------------------------------------------------------------------ pipeline (one C-ABI call each)
    def init_state(self):
        check(self.lib.dexsim_init_state(self.h, self._stream()), "init_state")

    def process_actions(self, actions, zero_targets=False):
        check(self.lib.dexsim_process_actions(self.h, self._actions_ptr(actions), int(zero_targets), self._stream()), "process_actions")

    def begin_step(self):
        """Open a control step whose action stage ran on the host (what dexsim_process_actions does for the device-side
        step bookkeeping: new reset-gate stamp, contact statistics words)."""
        check(self.lib.dexsim_begin_step(self.h, self._stream()), "begin_step")

    def physics_step(self, gate_on_reset=False):
        check(self.lib.dexsim_physics_step(self.h, int(gate_on_reset), self._stream()), "physics_step")

    def post_physics(self, obs_only=False):
        check(self.lib.dexsim_post_physics(self.h, int(obs_only), self._stream()), "post_physics")

    def step(self, actions):
        check(self.lib.dexsim_step(self.h, self._actions_ptr(actions), self._stream()), "step")

    def reset(self):
        check(self.lib.dexsim_reset(self.h, self._stream()), "reset")

    def reset_idx(self, env_ids):
        ptr, k = self._ids_ptr(env_ids)
        if k:
            check(self.lib.dexsim_reset_idx(self.h, ptr, k, self._stream()), "reset_idx")

    def refresh_body_states(self):
        check(self.lib.dexsim_refresh_body_states(self.h, self._stream()), "refresh_body_states")

    def set_dof_state_indexed(self, env_ids):
        ptr, k = self._ids_ptr(env_ids)
        check(self.lib.dexsim_set_dof_state_indexed(self.h, ptr, k, self._stream()), "set_dof_state_indexed")

    def set_root_state_indexed(self, env_ids):
        ptr, k = self._ids_ptr(env_ids)
        check(self.lib.dexsim_set_root_state_indexed(self.h, ptr, k, self._stream()), "set_root_state_indexed")

    def run_stage(self, stage):
        check(self.lib.dexsim_run_stage(self.h, int(stage), self._stream()), "run_stage")

    def set_step_sink(self, obs=None, rew=None, done=None):
        """Second destination of the next steps' outputs (rows of a rollout buffer): (N, O) f32, (N,) f32, (N,) u8 tensors
        on this device, contiguous; None switches a sink off.  The caller keeps the tensors alive."""
        def ptr(t, dtype, shape):
            if t is None:
                return None
            assert t.is_contiguous() and t.dtype == dtype and tuple(t.shape) == shape and t.device == self.device
            return C.c_void_p(t.data_ptr())
        self._sink_obs = obs                 # (env.py patches a custom pre-action rule's output into the sink row)
        check(self.lib.dexsim_set_step_sink(self.h, ptr(obs, torch.float32, (self.N, int(self.cfg.num_obs))),
                                            ptr(rew, torch.float32, (self.N,)), ptr(done, torch.uint8, (self.N,))), "set_step_sink")

    def set_obs_dict_mode(self, policy_only):
        """False: every obs_dict row is materialised each step (default); True: only obs_buf (the policy keys) is written."""
        check(self.lib.dexsim_set_obs_dict_mode(self.h, 1 if policy_only else 0), "set_obs_dict_mode")

    def set_phase_probe(self, on=True):
        """Switch the phase probe on (returns the zeroed (num_workgroups, 4) int32 tensor the kernels accumulate shader-clock
        ticks into: [:, 0] contact rows + sweeps, [:, 1] whole physics launch, [:, 2] general-path sub-steps, [:, 3] sweeps) or off."""
        self._probe = torch.zeros(self.NS // 64, 4, dtype=torch.int32, device=self.device) if on else None
        check(self.lib.dexsim_set_phase_probe(self.h, None if self._probe is None else C.c_void_p(self._probe.data_ptr())), "set_phase_probe")
        return self._probe

    def set_stats_sink(self, dst):
        """(STAT_WORDS,) f32 row that receives a copy of every step's statistics block (dexsim_set_stats_sink), or None."""
        if dst is not None:
            assert dst.is_contiguous() and dst.dtype == torch.float32 and dst.device == self.device and dst.numel() >= _abi.STAT_USED
        self._sink_stats = dst
        check(self.lib.dexsim_set_stats_sink(self.h, None if dst is None else C.c_void_p(dst.data_ptr())), "set_stats_sink")

    def set_action_copy(self, dst):
        """(N, num_actions) f32 tensor that receives a copy of every step's actions (DexHandBase.actions), or None."""
        if dst is not None:
            assert dst.is_contiguous() and dst.dtype == torch.float32 and dst.device == self.device
            assert tuple(dst.shape) == (self.N, int(self.cfg.num_actions))
        self._actions_copy = dst
        check(self.lib.dexsim_set_action_copy(self.h, None if dst is None else C.c_void_p(dst.data_ptr())), "set_action_copy")

    def step_timing(self, enable):
        """Start (True) / stop (False) the in-situ hipEvent timing of dexsim_step's main launch; stop returns (mean_us, n)."""
        us, n = C.c_float(0.0), C.c_int(0)
        check(self.lib.dexsim_step_timing(self.h, 1 if enable else 0, C.byref(us), C.byref(n)), "step_timing")
        return float(us.value), int(n.value)

    def time_stage(self, stage, launches):
        us = C.c_float(0)
        check(self.lib.dexsim_time_stage(self.h, int(stage), int(launches), self._stream(), C.byref(us)), "time_stage")
        return float(us.value)

    # ------------------------------------------------------------------ state records (save / load / fork)
    def state_layout(self):
        """({section name: (word offset inside a record, rows, is_int)}, record_words) -- dexsim_state_layout."""
        if getattr(self, "_state_layout", None) is None:      # fixed by the configuration: asked once
            fields = (_abi.DexSimField * 128)()
            nf, words = C.c_int(0), C.c_size_t(0)
            check(self.lib.dexsim_state_layout(C.byref(self.cfg), fields, 128, C.byref(nf), C.byref(words)), "state_layout")
            self._state_layout = ({fields[i].name.decode(): (int(fields[i].offset), int(fields[i].rows), bool(fields[i].is_int))
                                   for i in range(nf.value)}, int(words.value))
        return self._state_layout

    def state_bank(self, capacity):
        """A zeroed StateBank of `capacity` slots on this device (record_words * pad64(capacity) * 4 bytes)."""
        layout, words = self.state_layout()
        capacity = int(capacity)
        if capacity <= 0:
            raise DexSimError(f"state_bank: capacity must be positive, got {capacity}")
        data = torch.zeros(words * ((capacity + 63) // 64 * 64), dtype=torch.float32, device=self.device)
        return StateBank(data, capacity, words, layout)

    def _bank_args(self, bank, env_ids, slots, what):
        if not isinstance(bank, StateBank):
            raise DexSimError(f"{what}: bank must be a StateBank (DexSimCore.state_bank)")
        _, words = self.state_layout()
        if bank.version != _abi.STATE_VERSION:
            raise DexSimError(f"{what}: state bank has version {bank.version}, this library writes version {_abi.STATE_VERSION}")
        if bank.record_words != words:
            raise DexSimError(f"{what}: state bank has record_words {bank.record_words}, this configuration needs {words}")
        d = bank.data
        if d.device != self.device or d.dtype != torch.float32 or not d.is_contiguous() or d.numel() != words * bank.stride:
            raise DexSimError(f"{what}: the bank tensor must be contiguous float32 on {self.device} with record_words * pad64(capacity) elements")
        if env_ids is None and slots is None:
            return None, None, 0
        if env_ids is None or slots is None:     # one side given: the other side counts 0, 1, 2, ...
            n = len(slots if env_ids is None else env_ids)
            rng = torch.arange(n, device=self.device)
            env_ids, slots = (rng if env_ids is None else env_ids), (rng if slots is None else slots)
        e = torch.as_tensor(env_ids, device=self.device).to(torch.int64).contiguous().view(-1)
        s = torch.as_tensor(slots, device=self.device).to(torch.int64).contiguous().view(-1)
        if e.numel() != s.numel():
            raise DexSimError(f"{what}: {e.numel()} env ids but {s.numel()} slots")
        self._keep_state_ids = (e, s)
        return e, s, int(e.numel())

    def save_state(self, bank, env_ids=None, slots=None):
        """Records of `env_ids` -> bank slots `slots` (dexsim_save_state); both None = every lane to the slot of its own index."""
        e, s, k = self._bank_args(bank, env_ids, slots, "save_state")
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        check(self.lib.dexsim_save_state(self.h, ptr(e), ptr(s), k, C.c_void_p(bank.data.data_ptr()), bank.capacity, self._stream()), "save_state")

    def load_state(self, bank, env_ids=None, slots=None):
        """Bank slots `slots` -> records of `env_ids` (dexsim_load_state); env_ids must not repeat."""
        e, s, k = self._bank_args(bank, env_ids, slots, "load_state")
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        check(self.lib.dexsim_load_state(self.h, ptr(e), ptr(s), k, C.c_void_p(bank.data.data_ptr()), bank.capacity, self._stream()), "load_state")

    def copy_envs(self, src_ids, dst_ids):
        """Fork: record of env src_ids[i] -> env dst_ids[i] (dexsim_copy_envs).  Precondition, not checked here: the
        destinations are unique and disjoint from the sources (DexHandEnv.fork_envs checks it)."""
        a = torch.as_tensor(src_ids, device=self.device).to(torch.int64).contiguous().view(-1)
        b = torch.as_tensor(dst_ids, device=self.device).to(torch.int64).contiguous().view(-1)
        if a.numel() != b.numel():
            raise DexSimError(f"copy_envs: {a.numel()} sources but {b.numel()} destinations")
        self._keep_state_ids = (a, b)
        check(self.lib.dexsim_copy_envs(self.h, C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), int(a.numel()), self._stream()), "copy_envs")

    def get_step_stamp(self):
        v = C.c_int(0)
        check(self.lib.dexsim_get_step_stamp(self.h, C.byref(v)), "get_step_stamp")
        return int(v.value)

    def set_step_stamp(self, stamp):
        check(self.lib.dexsim_set_step_stamp(self.h, int(stamp)), "set_step_stamp")

    # ------------------------------------------------------------------ camera sensors (dexsim_render)
    def render_layout(self):
        """({section name: (word offset inside a scene record, words, is_int)}, scene_words) -- dexsim_render_layout."""
        if getattr(self, "_render_layout", None) is None:
            fields = (_abi.DexSimField * 32)()
            nf, words = C.c_int(0), C.c_size_t(0)
            check(self.lib.dexsim_render_layout(fields, 32, C.byref(nf), C.byref(words)), "render_layout")
            self._render_layout = ({fields[i].name.decode(): (int(fields[i].offset), int(fields[i].rows), bool(fields[i].is_int))
                                    for i in range(nf.value)}, int(words.value))
        return self._render_layout

    def render(self, cam, scene, depth=None, rgba=None, seg=None, env_ids=None, eye=None, target=None):
        """Render `cam` (an _abi.DexSimCamera) for the envs `env_ids` (None = all) into the caller's tensors: scene
        (k, scene_words) f32 workspace, depth (k, H, W) f32, rgba (k, H, W, 4) u8, seg (k, H, W) i32 (any output may be None, not
        all); eye / target: optional (k, 3) f32 per-env overrides of the camera's look-at pair.  All on this device, contiguous."""
        _, words = self.render_layout()
        H, W = int(cam.height), int(cam.width)
        ids = None
        k = self.N
        if env_ids is not None:
            ids = torch.as_tensor(env_ids, device=self.device).to(torch.int64).contiguous().view(-1)
            k = int(ids.numel())

        def ptr(t, name, dtype, shape, optional=True):
            if t is None:
                if optional:
                    return None
                raise DexSimError(f"render: {name} is required")
            if t.device != self.device or t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != shape:
                raise DexSimError(f"render: {name} must be a contiguous {dtype} tensor of shape {shape} on {self.device}, "
                                  f"got {t.dtype} {tuple(t.shape)} on {t.device}")
            return C.c_void_p(t.data_ptr())
        if depth is None and rgba is None and seg is None:
            raise DexSimError("render: at least one of depth, rgba and seg is required")
        args = (ptr(eye, "eye", torch.float32, (k, 3)), ptr(target, "target", torch.float32, (k, 3)),
                None if ids is None else C.c_void_p(ids.data_ptr()), k,
                ptr(scene, "scene", torch.float32, (k, words), optional=False),
                ptr(depth, "depth", torch.float32, (k, H, W)), ptr(rgba, "rgba", torch.uint8, (k, H, W, 4)),
                ptr(seg, "seg", torch.int32, (k, H, W)))
        self._keep_render = (ids, eye, target)     # alive until the kernels ran
        check(self.lib.dexsim_render(self.h, C.byref(cam), *args, self._stream()), "render")

    # ------------------------------------------------------------------ Jacobians, mass matrix, gravity force
    def _kin_rows(self, what, env_ids, q):
        """(ids pointer, q pointer, k) of a dexsim_body_jacobian / dexsim_mass_matrix call; keeps the tensors alive."""
        ids = None
        k = self.N
        if q is not None:
            if q.device != self.device or q.dtype != torch.float32 or not q.is_contiguous() or q.dim() != 2 or q.shape[1] != _abi.NJ \
                    or q.shape[0] < 1:
                raise DexSimError(f"{what}: q must be a contiguous float32 tensor of shape (k, {_abi.NJ}), k >= 1, on {self.device}, "
                                  f"got {q.dtype} {tuple(q.shape)} on {q.device}")
            k = int(q.shape[0])
        elif env_ids is not None:
            ids = torch.as_tensor(env_ids, device=self.device).to(torch.int64).contiguous().view(-1)
            k = int(ids.numel())
            if k < 1:
                raise DexSimError(f"{what}: env_ids is empty")
        self._keep_kin = (ids, q)
        return (None if ids is None else C.c_void_p(ids.data_ptr())), (None if q is None else C.c_void_p(q.data_ptr())), k

    def _kin_out(self, what, name, t, shape):
        if t.device != self.device or t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape:
            raise DexSimError(f"{what}: {name} must be a contiguous float32 tensor of shape {shape} on {self.device}, "
                              f"got {t.dtype} {tuple(t.shape)} on {t.device}")
        return C.c_void_p(t.data_ptr())

    def _kin_bodies(self, what, bodies):
        """(nb, c_int array or None = all 37) of a body list."""
        if bodies is None:
            return _abi.NUM_HAND_BODIES, None
        bl = [int(b) for b in bodies]
        nb = len(bl)
        if not 1 <= nb <= _abi.NUM_HAND_BODIES:
            raise DexSimError(f"{what}: between 1 and {_abi.NUM_HAND_BODIES} bodies, got {nb}")
        return nb, (C.c_int * nb)(*bl)

    def body_jacobian(self, out, env_ids=None, q=None, bodies=None):
        """Geometric Jacobians of the hand bodies `bodies` (indices into the rows of rigid_body_states; None = all 37) into
        `out` (k, nb, 6, 26) f32: rows 0-2 linear velocity of the body origin, 3-5 angular velocity, world frame, so that
        out[i, b] @ qd == rigid_body_states[env, b, 7:13].  Rows: env_ids (None = all envs), or the rows of a (k, 26) `q`
        override (env_ids is then ignored).  dexsim_body_jacobian."""
        ids, qp, k = self._kin_rows("body_jacobian", env_ids, q)
        nb, bp = self._kin_bodies("body_jacobian", bodies)
        op = self._kin_out("body_jacobian", "out", out, (k, nb, 6, _abi.NJ))
        check(self.lib.dexsim_body_jacobian(self.h, ids, k, qp, bp, nb, op, self._stream()), "body_jacobian")

    def mass_matrix(self, mass=None, gravity=None, env_ids=None, q=None):
        """Joint-space inertia M(q) into `mass` (k, 26, 26) f32 and / or the gravity force dV/dq into `gravity` (k, 26) f32
        (what a controller adds to hold the hand).  M carries no armature and no PD terms.  Rows as for body_jacobian.
        dexsim_mass_matrix."""
        if mass is None and gravity is None:
            raise DexSimError("mass_matrix: at least one of mass and gravity is required")
        ids, qp, k = self._kin_rows("mass_matrix", env_ids, q)
        mp = None if mass is None else self._kin_out("mass_matrix", "mass", mass, (k, _abi.NJ, _abi.NJ))
        gp = None if gravity is None else self._kin_out("mass_matrix", "gravity", gravity, (k, _abi.NJ))
        check(self.lib.dexsim_mass_matrix(self.h, ids, k, qp, mp, gp, self._stream()), "mass_matrix")

    # ------------------------------------------------------------------ inverse dynamics, bias accelerations
    def _kin_vel(self, what, name, t, k):
        """Pointer of a (k, 26) velocity or acceleration array that goes with the rows of _kin_rows; checked like q."""
        if t.device != self.device or t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (k, _abi.NJ):
            raise DexSimError(f"{what}: {name} must be a contiguous float32 tensor of shape ({k}, {_abi.NJ}) on {self.device}, "
                              f"got {t.dtype} {tuple(t.shape)} on {t.device}")
        return C.c_void_p(t.data_ptr())

    def _kin_rows_qd(self, what, env_ids, q, qd):
        if (q is None) != (qd is None):
            raise DexSimError(f"{what}: q and qd must both be None (the envs' state) or both be (k, {_abi.NJ}) overrides")
        ids, qp, k = self._kin_rows(what, env_ids, q)
        return ids, qp, (None if qd is None else self._kin_vel(what, "qd", qd, k)), k

    def inverse_dynamics(self, tau, qdd=None, env_ids=None, q=None, qd=None, gravity=True):
        """tau = M(q) qdd + c(q, qd) (+ g(q) with gravity=True) into `tau` (k, 26) f32, with the M and g of mass_matrix (no
        armature, no PD terms, no contact).  qdd: (k, 26) aligned with the output rows, None = zero (tau is then the bias force).
        Rows: env_ids (None = all envs) with the envs' q and qd, or the rows of the (k, 26) overrides `q` and `qd`, which go
        together (env_ids is then ignored).  dexsim_inverse_dynamics."""
        ids, qp, vp, k = self._kin_rows_qd("inverse_dynamics", env_ids, q, qd)
        ap = None if qdd is None else self._kin_vel("inverse_dynamics", "qdd", qdd, k)
        tp = self._kin_out("inverse_dynamics", "tau", tau, (k, _abi.NJ))
        self._keep_kin = self._keep_kin + (qd, qdd)
        check(self.lib.dexsim_inverse_dynamics(self.h, ids, k, qp, vp, ap, _abi.ID_GRAVITY if gravity else 0, tp, self._stream()),
              "inverse_dynamics")

    def body_bias_accel(self, out, env_ids=None, q=None, qd=None, bodies=None):
        """Jdot qd of the hand bodies `bodies` (None = all 37) into `out` (k, nb, 6) f32: world linear acceleration of the body
        origin (0-2) and angular acceleration (3-5) at qdd = 0, without gravity, so that body_jacobian's out[i, b] @ qdd + this
        is the derivative of rigid_body_states[env, b, 7:13].  Rows as for inverse_dynamics.  dexsim_body_bias_accel."""
        ids, qp, vp, k = self._kin_rows_qd("body_bias_accel", env_ids, q, qd)
        nb, bp = self._kin_bodies("body_bias_accel", bodies)
        op = self._kin_out("body_bias_accel", "out", out, (k, nb, 6))
        self._keep_kin = self._keep_kin + (qd,)
        check(self.lib.dexsim_body_bias_accel(self.h, ids, k, qp, vp, bp, nb, op, self._stream()), "body_bias_accel")

    # ------------------------------------------------------------------ forward dynamics, mass-matrix solves
    def forward_dynamics(self, out, tau=None, env_ids=None, q=None, qd=None, gravity=True, armature=False):
        """qdd = (M(q) [+ A])^-1 (tau - c(q, qd) [- g(q)]) into `out` (k, 26) f32, with the M, c and g of mass_matrix and
        inverse_dynamics; armature=True solves with M + diag(model.armature).  tau: (k, 26) aligned with the output rows,
        None = zero (out is then the free acceleration).  Rows as for inverse_dynamics.  dexsim_forward_dynamics."""
        ids, qp, vp, k = self._kin_rows_qd("forward_dynamics", env_ids, q, qd)
        tp = None if tau is None else self._kin_vel("forward_dynamics", "tau", tau, k)
        op = self._kin_out("forward_dynamics", "out", out, (k, _abi.NJ))
        self._keep_kin = self._keep_kin + (qd, tau)
        flags = (_abi.FD_GRAVITY if gravity else 0) | (_abi.FD_ARMATURE if armature else 0)
        check(self.lib.dexsim_forward_dynamics(self.h, ids, k, qp, vp, tp, flags, op, self._stream()), "forward_dynamics")

    def mass_solve(self, out, rhs, env_ids=None, q=None, armature=False):
        """out[i, r] = (M(q_i) [+ A])^-1 rhs[i, r] for `rhs` and `out` (k, nrhs, 26) f32, nrhs in [1, 32]; a row is factored once.
        `out` may be `rhs` itself (in place).  Rows as for mass_matrix.  dexsim_mass_solve."""
        ids, qp, k = self._kin_rows("mass_solve", env_ids, q)
        if rhs.dim() != 3 or not 1 <= rhs.shape[1] <= _abi.MSOLVE_MAX_RHS:
            raise DexSimError(f"mass_solve: rhs must have shape ({k}, nrhs, {_abi.NJ}) with nrhs in [1, {_abi.MSOLVE_MAX_RHS}], "
                              f"got {tuple(rhs.shape)}")
        nrhs = int(rhs.shape[1])
        rp = self._kin_out("mass_solve", "rhs", rhs, (k, nrhs, _abi.NJ))
        op = self._kin_out("mass_solve", "out", out, (k, nrhs, _abi.NJ))
        self._keep_kin = self._keep_kin + (rhs,)
        check(self.lib.dexsim_mass_solve(self.h, ids, k, qp, rp, nrhs, _abi.FD_ARMATURE if armature else 0, op, self._stream()),
              "mass_solve")

    # ------------------------------------------------------------------ derivatives of the inverse and the forward dynamics
    def _kin_deriv_outs(self, what, names, outs, k):
        if all(o is None for o in outs):
            raise DexSimError(f"{what}: at least one of {names[0]} and {names[1]} is required")
        return [None if o is None else self._kin_out(what, n, o, (k, _abi.NJ, _abi.NJ)) for n, o in zip(names, outs)]

    def inverse_dynamics_derivatives(self, dtau_dq=None, dtau_dqd=None, qdd=None, env_ids=None, q=None, qd=None, gravity=True):
        """The derivatives of inverse_dynamics at fixed qdd into `dtau_dq` and / or `dtau_dqd`, each (k, 26, 26) f32 and
        derivative-major: out[i, c, r] = d tau_r / d (q or qd)_c (the transpose of the Jacobian).  Either may be None, not both.
        qdd and rows as for inverse_dynamics.  dexsim_inverse_dynamics_derivatives."""
        what = "inverse_dynamics_derivatives"
        ids, qp, vp, k = self._kin_rows_qd(what, env_ids, q, qd)
        ap = None if qdd is None else self._kin_vel(what, "qdd", qdd, k)
        dp, dvp = self._kin_deriv_outs(what, ("dtau_dq", "dtau_dqd"), (dtau_dq, dtau_dqd), k)
        self._keep_kin = self._keep_kin + (qd, qdd)
        check(self.lib.dexsim_inverse_dynamics_derivatives(self.h, ids, k, qp, vp, ap, _abi.ID_GRAVITY if gravity else 0, dp, dvp,
                                                           self._stream()), what)

    def forward_dynamics_derivatives(self, qdd, dqdd_dq=None, dqdd_dqd=None, tau=None, env_ids=None, q=None, qd=None, gravity=True,
                                     armature=False):
        """forward_dynamics into `qdd` (k, 26) f32 (required) and its derivatives at fixed tau into `dqdd_dq` and / or `dqdd_dqd`,
        (k, 26, 26) f32, derivative-major: out[i, c, r] = d qdd_r / d (q or qd)_c.  tau, flags and rows as for forward_dynamics.
        dexsim_forward_dynamics_derivatives."""
        what = "forward_dynamics_derivatives"
        ids, qp, vp, k = self._kin_rows_qd(what, env_ids, q, qd)
        tp = None if tau is None else self._kin_vel(what, "tau", tau, k)
        op = self._kin_out(what, "qdd", qdd, (k, _abi.NJ))
        dp, dvp = self._kin_deriv_outs(what, ("dqdd_dq", "dqdd_dqd"), (dqdd_dq, dqdd_dqd), k)
        self._keep_kin = self._keep_kin + (qd, tau)
        flags = (_abi.FD_GRAVITY if gravity else 0) | (_abi.FD_ARMATURE if armature else 0)
        check(self.lib.dexsim_forward_dynamics_derivatives(self.h, ids, k, qp, vp, tp, flags, op, dp, dvp, self._stream()), what)

    # ------------------------------------------------------------------ fingertip inverse kinematics
    def solve_ik(self, targets, controls, env_ids=None, q=None, sites=0, frame=0, free_mask=0x3FFC0, weights=(1, 1, 1, 1, 1),
                 iters=16, damping=1e-3, max_step=0.5, q_out=None, residual=None):
        """Damped-least-squares IK of the five fingertip (sites=0) or fingerpad (sites=1) positions in control space, all `iters`
        iterations in one launch: `targets` (k, 5, 3) f32 in the world (frame=0) or hand (frame=1) frame -> `controls` (k, 18) f32,
        the 18 active targets of the action stage; optionally `q_out` (k, 26) = the coupled joint positions and `residual` (k, 5)
        = |target - site| per finger.  Bit c of free_mask: control c is an unknown.  Rows as for body_jacobian: env_ids (None =
        all envs) start from their current q, the rows of a (k, 26) `q` override from that.  dexsim_solve_ik."""
        ids, qp, k = self._kin_rows("solve_ik", env_ids, q)
        prm = _abi.DexSimIK()
        prm.sites, prm.frame, prm.free_mask, prm.iters = int(sites), int(frame), int(free_mask), int(iters)
        prm.damping, prm.max_step = float(damping), float(max_step)
        w = [float(x) for x in weights]
        if len(w) != _abi.NFINGER:
            raise DexSimError(f"solve_ik: {_abi.NFINGER} weights, got {len(w)}")
        prm.weight[:] = w
        tp = self._kin_out("solve_ik", "targets", targets, (k, _abi.NFINGER, 3))
        cp = self._kin_out("solve_ik", "controls", controls, (k, _abi.NACT))
        qo = None if q_out is None else self._kin_out("solve_ik", "q_out", q_out, (k, _abi.NJ))
        rp = None if residual is None else self._kin_out("solve_ik", "residual", residual, (k, _abi.NFINGER))
        self._keep_ik = targets                     # alive until the kernel ran
        check(self.lib.dexsim_solve_ik(self.h, ids, k, qp, tp, C.byref(prm), cp, qo, rp, self._stream()), "solve_ik")

    # ------------------------------------------------------------------ clearance queries
    def proximity_pairs(self):
        """The pair table of dexsim_query_proximity as a list of NPROX_PAIRS (capsule A, capsule B, group) triples."""
        a, b, g = C.c_int(0), C.c_int(0), C.c_int(0)
        out = []
        for i in range(_abi.NPROX_PAIRS):
            check(self.lib.dexsim_proximity_pair(i, C.byref(a), C.byref(b), C.byref(g)), "proximity_pair")
            out.append((a.value, b.value, g.value))
        return out

    def proximity(self, cap_env=None, self_min=None, pair_dist=None, env_ids=None, q=None, box_pose=None, box_size=0.0):
        """Clearances of the hand in one launch: `cap_env` (k, 18, 2, 8) f32 = every collision capsule against the box (record 0) and
        the ground plane (record 1) as (signed distance, normal towards the capsule, witness on the other shape, axis parameter);
        `self_min` (k, 15, 8) = the closest capsule pair of every finger pair and of the palm with every finger; `pair_dist`
        (k, 120) = the distance of every pair of the pair table.  Any of the three may be None, not all.  Rows as for body_jacobian:
        env_ids (None = all envs), or the rows of a (k, 26) `q` override.  The box: `box_pose` (k, 7) f32 (centre, quaternion xyzw)
        when given, else the env's own box on the state path, else none; `box_size` > 0 overrides cfg.box_size.
        dexsim_query_proximity."""
        if cap_env is None and self_min is None and pair_dist is None:
            raise DexSimError("proximity: at least one of cap_env, self_min and pair_dist is required")
        ids, qp, k = self._kin_rows("proximity", env_ids, q)
        bp = None if box_pose is None else self._kin_out("proximity", "box_pose", box_pose, (k, 7))
        cp = None if cap_env is None else self._kin_out("proximity", "cap_env", cap_env, (k, _abi.NCAP, 2, 8))
        sp = None if self_min is None else self._kin_out("proximity", "self_min", self_min, (k, _abi.NPROX_GROUPS, 8))
        pp = None if pair_dist is None else self._kin_out("proximity", "pair_dist", pair_dist, (k, _abi.NPROX_PAIRS))
        self._keep_prox = box_pose                  # alive until the kernel ran
        check(self.lib.dexsim_query_proximity(self.h, ids, k, qp, bp, float(box_size), cp, sp, pp, self._stream()), "query_proximity")
