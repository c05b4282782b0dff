"""The query surface: everything that reads or copies simulation state outside the control step -- state records (save, load,
fork), camera sensors, Jacobians and mass matrix, inverse dynamics, forward kinematics, forward dynamics and the dynamics
derivatives, fingertip IK, clearances, range sensors.

Two levels, in the same family order.  CoreQueries, a base class of DexSimCore, is the ctypes level: one C-ABI call per method
on caller-owned device tensors, DexSimError on a bad argument.  EnvQueries, a base class of DexHandEnv, is the user level: it
accepts lists, names and arrays, allocates the outputs and raises ValueError.  The argument rules that every call repeats are
written once, at the top of this file and at the top of each class.  A new query adds a method to each class (and its row to
_abi.PROTOTYPES, or to the table of the header part that declares it: _abi.FK_PROTOTYPES for include/dexsim_fk.h, _abi.RAY_PROTOTYPES
for include/dexsim_ray.h); nothing else."""
import ctypes as C
import hashlib

import numpy as np
import torch

from . import _abi
from ._lib import DexSimError, check
from .config import FINGER_COUPLING_MAP, HARDWARE_MAPPING


def env_id_vector(ids, device):
    """A list, array or tensor of env ids (or bank slots) as a flat contiguous int64 vector on `device`."""
    return torch.as_tensor(ids, device=device).to(torch.int64).contiguous().view(-1)


def field_table(layout_call, what, max_fields, *args):
    """({name: (offset, rows, is_int)}, total words) of a DexSimField table: dexsim_arena_layout / _state_layout / _render_layout."""
    fields = (_abi.DexSimField * max_fields)()
    nf, words = C.c_int(0), C.c_size_t(0)
    check(layout_call(*args, fields, max_fields, C.byref(nf), C.byref(words)), what)
    return {f.name.decode(): (int(f.offset), int(f.rows), bool(f.is_int)) for f in fields[:nf.value]}, int(words.value)


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


Q_ROWS = f"a contiguous float32 tensor of shape (k, {_abi.NJ}), k >= 1,"     # how the calls word the shape of a q override


class CoreQueries:
    """The ctypes level of the queries.  DexSimCore supplies lib, h, cfg, device, N and _stream()."""

    # ------------------------------------------------------------------ the argument rules
    def _opt(self, what, name, t, shape, dtype=torch.float32, required=False, wording=None, error=DexSimError):
        """The device pointer of the tensor argument `name` of the call `what` after the check every entry point makes: a
        contiguous `dtype` tensor of shape `shape` on this device, else `error`.  None gives NULL, or `error` when `required`.
        `wording` replaces the shape rule in the text where it is not a plain shape."""
        if t is None:
            if required:
                raise error(f"{what}: {name} is required")
            return None
        if t.device != self.device or t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != shape:
            wording = wording or f"a contiguous {str(dtype).replace('torch.', '')} tensor of shape {shape}"
            raise error(f"{what}: {name} must be {wording} on {self.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
        return C.c_void_p(t.data_ptr())

    def _req(self, what, name, t, shape):
        return self._opt(what, name, t, shape, required=True)

    # ------------------------------------------------------------------ state records (save / load / fork)
    def state_layout(self):
        """({section name: (word offset inside a record, rows, is_int)}, record_words) -- dexsim_state_layout."""
        if getattr(self, "_state_layout", None) is None:      # fixed by the configuration: asked once
            self._state_layout = field_table(self.lib.dexsim_state_layout, "state_layout", 128, C.byref(self.cfg))
        return self._state_layout

    def state_bank(self, capacity):
        """A zeroed StateBank of `capacity` slots on this device (record_words * pad64(capacity) * 4 bytes)."""
        layout, words = self.state_layout()
        capacity = int(capacity)
        if capacity <= 0:
            raise DexSimError(f"state_bank: capacity must be positive, got {capacity}")
        data = torch.zeros(words * ((capacity + 63) // 64 * 64), dtype=torch.float32, device=self.device)
        return StateBank(data, capacity, words, layout)

    def _bank_transfer(self, what, bank, env_ids, slots):
        """dexsim_save_state / dexsim_load_state (`what` without the prefix): the two differ in the direction only."""
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
        ep, sp, k = None, None, 0
        if env_ids is not None or slots is not None:
            if env_ids is None or slots is None:     # one side given: the other side counts 0, 1, 2, ...
                n = len(slots if env_ids is None else env_ids)
                rng = torch.arange(n, device=self.device)
                env_ids, slots = (rng if env_ids is None else env_ids), (rng if slots is None else slots)
            e, s = env_id_vector(env_ids, self.device), env_id_vector(slots, self.device)
            if e.numel() != s.numel():
                raise DexSimError(f"{what}: {e.numel()} env ids but {s.numel()} slots")
            self._keep_state_ids = (e, s)
            ep, sp, k = C.c_void_p(e.data_ptr()), C.c_void_p(s.data_ptr()), int(e.numel())
        check(getattr(self.lib, "dexsim_" + what)(self.h, ep, sp, k, C.c_void_p(d.data_ptr()), bank.capacity, self._stream()), what)

    def save_state(self, bank, env_ids=None, slots=None):
        """Records of `env_ids` -> bank slots `slots` (dexsim_save_state); both None = every lane to the slot of its own index."""
        self._bank_transfer("save_state", bank, env_ids, slots)

    def load_state(self, bank, env_ids=None, slots=None):
        """Bank slots `slots` -> records of `env_ids` (dexsim_load_state); env_ids must not repeat."""
        self._bank_transfer("load_state", bank, env_ids, slots)

    def copy_envs(self, src_ids, dst_ids):
        """Fork: record of env src_ids[i] -> env dst_ids[i] (dexsim_copy_envs).  Precondition, not checked here: the
        destinations are unique and disjoint from the sources (DexHandEnv.fork_envs checks it)."""
        a, b = env_id_vector(src_ids, self.device), env_id_vector(dst_ids, self.device)
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
            self._render_layout = field_table(self.lib.dexsim_render_layout, "render_layout", 32)
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
            ids = env_id_vector(env_ids, self.device)
            k = int(ids.numel())

        def ptr(t, name, dtype, shape, required=False):     # this family names the dtype as torch does
            return self._opt("render", name, t, shape, dtype, required, f"a contiguous {dtype} tensor of shape {shape}")
        if depth is None and rgba is None and seg is None:
            raise DexSimError("render: at least one of depth, rgba and seg is required")
        args = (ptr(eye, "eye", torch.float32, (k, 3)), ptr(target, "target", torch.float32, (k, 3)),
                None if ids is None else C.c_void_p(ids.data_ptr()), k,
                ptr(scene, "scene", torch.float32, (k, words), required=True),
                ptr(depth, "depth", torch.float32, (k, H, W)), ptr(rgba, "rgba", torch.uint8, (k, H, W, 4)),
                ptr(seg, "seg", torch.int32, (k, H, W)))
        self._keep_render = (ids, eye, target)     # alive until the kernels ran
        check(self.lib.dexsim_render(self.h, C.byref(cam), *args, self._stream()), "render")

    # ------------------------------------------------------------------ Jacobians, mass matrix, gravity force
    def _kin_rows(self, what, env_ids, q):
        """(ids pointer, q pointer, k) of a dexsim_body_jacobian / dexsim_mass_matrix call; keeps the tensors alive."""
        ids, qp = None, None
        k = self.N
        if q is not None:
            k = int(q.shape[0]) if q.dim() == 2 else 0
            qp = self._opt(what, "q", q, (max(k, 1), _abi.NJ), wording=Q_ROWS)
        elif env_ids is not None:
            ids = env_id_vector(env_ids, self.device)
            k = int(ids.numel())
            if k < 1:
                raise DexSimError(f"{what}: env_ids is empty")
        self._keep_kin = (ids, q)
        return (None if ids is None else C.c_void_p(ids.data_ptr())), qp, k

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
        op = self._req("body_jacobian", "out", out, (k, nb, 6, _abi.NJ))
        check(self.lib.dexsim_body_jacobian(self.h, ids, k, qp, bp, nb, op, self._stream()), "body_jacobian")

    def mass_matrix(self, mass=None, gravity=None, env_ids=None, q=None):
        """Joint-space inertia M(q) into `mass` (k, 26, 26) f32 and / or the gravity force dV/dq into `gravity` (k, 26) f32
        (what a controller adds to hold the hand).  M carries no armature and no PD terms.  Rows as for body_jacobian.
        dexsim_mass_matrix."""
        if mass is None and gravity is None:
            raise DexSimError("mass_matrix: at least one of mass and gravity is required")
        ids, qp, k = self._kin_rows("mass_matrix", env_ids, q)
        mp = self._opt("mass_matrix", "mass", mass, (k, _abi.NJ, _abi.NJ))
        gp = self._opt("mass_matrix", "gravity", gravity, (k, _abi.NJ))
        check(self.lib.dexsim_mass_matrix(self.h, ids, k, qp, mp, gp, self._stream()), "mass_matrix")

    # ------------------------------------------------------------------ inverse dynamics, bias accelerations
    def _kin_rows_qd(self, what, env_ids, q, qd):
        if (q is None) != (qd is None):
            raise DexSimError(f"{what}: q and qd must both be None (the envs' state) or both be (k, {_abi.NJ}) overrides")
        ids, qp, k = self._kin_rows(what, env_ids, q)
        return ids, qp, self._opt(what, "qd", qd, (k, _abi.NJ)), k

    def inverse_dynamics(self, tau, qdd=None, env_ids=None, q=None, qd=None, gravity=True):
        """tau = M(q) qdd + c(q, qd) (+ g(q) with gravity=True) into `tau` (k, 26) f32, with the M and g of mass_matrix (no
        armature, no PD terms, no contact).  qdd: (k, 26) aligned with the output rows, None = zero (tau is then the bias force).
        Rows: env_ids (None = all envs) with the envs' q and qd, or the rows of the (k, 26) overrides `q` and `qd`, which go
        together (env_ids is then ignored).  dexsim_inverse_dynamics."""
        ids, qp, vp, k = self._kin_rows_qd("inverse_dynamics", env_ids, q, qd)
        ap = self._opt("inverse_dynamics", "qdd", qdd, (k, _abi.NJ))
        tp = self._req("inverse_dynamics", "tau", tau, (k, _abi.NJ))
        self._keep_kin = self._keep_kin + (qd, qdd)
        check(self.lib.dexsim_inverse_dynamics(self.h, ids, k, qp, vp, ap, _abi.ID_GRAVITY if gravity else 0, tp, self._stream()),
              "inverse_dynamics")

    def body_bias_accel(self, out, env_ids=None, q=None, qd=None, bodies=None):
        """Jdot qd of the hand bodies `bodies` (None = all 37) into `out` (k, nb, 6) f32: world linear acceleration of the body
        origin (0-2) and angular acceleration (3-5) at qdd = 0, without gravity, so that body_jacobian's out[i, b] @ qdd + this
        is the derivative of rigid_body_states[env, b, 7:13].  Rows as for inverse_dynamics.  dexsim_body_bias_accel."""
        ids, qp, vp, k = self._kin_rows_qd("body_bias_accel", env_ids, q, qd)
        nb, bp = self._kin_bodies("body_bias_accel", bodies)
        op = self._req("body_bias_accel", "out", out, (k, nb, 6))
        self._keep_kin = self._keep_kin + (qd,)
        check(self.lib.dexsim_body_bias_accel(self.h, ids, k, qp, vp, bp, nb, op, self._stream()), "body_bias_accel")

    # ------------------------------------------------------------------ forward kinematics
    def forward_kinematics(self, body_states=None, site_poses=None, centroid=None, env_ids=None, q=None, qd=None, bodies=None,
                           hand_frame=False):
        """The configuration in one launch: `body_states` (k, nb, 13) f32 = rows of rigid_body_states for the hand bodies `bodies`
        (None = all 37); `site_poses` (k, 11, 7) f32 = position and quaternion xyzw of right_hand_base, the five tips and the five
        pads, in the world frame or, with hand_frame=True, relative to right_hand_base; `centroid` (k, 8) f32 = centre of mass,
        potential energy, velocity of the centre of mass, kinetic energy.  Any of the three may be None, not all.  Rows as for
        body_jacobian; with a `q` override `qd` is an optional (k, 26) override, None = every velocity word is +0.0; without `q`
        the velocities are the envs' and `qd` must be None.  dexsim_forward_kinematics."""
        what = "forward_kinematics"
        if body_states is None and site_poses is None and centroid is None:
            raise DexSimError(f"{what}: at least one of body_states, site_poses and centroid is required")
        if qd is not None and q is None:
            raise DexSimError(f"{what}: a qd override needs a q override (without q the velocities are the envs')")
        ids, qp, k = self._kin_rows(what, env_ids, q)
        vp = self._opt(what, "qd", qd, (k, _abi.NJ))
        nb, bp = (0, None) if body_states is None else self._kin_bodies(what, bodies)
        op = self._opt(what, "body_states", body_states, (k, nb, 13))
        sp = self._opt(what, "site_poses", site_poses, (k, _abi.NSITE, 7))
        cp = self._opt(what, "centroid", centroid, (k, 8))
        self._keep_kin = self._keep_kin + (qd,)
        check(self.lib.dexsim_forward_kinematics(self.h, ids, k, qp, vp, bp, nb, _abi.FK_HAND_FRAME if hand_frame else 0, op, sp, cp,
                                                 self._stream()), what)

    # ------------------------------------------------------------------ forward dynamics, mass-matrix solves
    def forward_dynamics(self, out, tau=None, env_ids=None, q=None, qd=None, gravity=True, armature=False):
        """qdd = (M(q) [+ A])^-1 (tau - c(q, qd) [- g(q)]) into `out` (k, 26) f32, with the M, c and g of mass_matrix and
        inverse_dynamics; armature=True solves with M + diag(model.armature).  tau: (k, 26) aligned with the output rows,
        None = zero (out is then the free acceleration).  Rows as for inverse_dynamics.  dexsim_forward_dynamics."""
        ids, qp, vp, k = self._kin_rows_qd("forward_dynamics", env_ids, q, qd)
        tp = self._opt("forward_dynamics", "tau", tau, (k, _abi.NJ))
        op = self._req("forward_dynamics", "out", out, (k, _abi.NJ))
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
        rp = self._req("mass_solve", "rhs", rhs, (k, nrhs, _abi.NJ))
        op = self._req("mass_solve", "out", out, (k, nrhs, _abi.NJ))
        self._keep_kin = self._keep_kin + (rhs,)
        check(self.lib.dexsim_mass_solve(self.h, ids, k, qp, rp, nrhs, _abi.FD_ARMATURE if armature else 0, op, self._stream()),
              "mass_solve")

    # ------------------------------------------------------------------ derivatives of the inverse and the forward dynamics
    def _kin_deriv_outs(self, what, names, outs, k):
        if all(o is None for o in outs):
            raise DexSimError(f"{what}: at least one of {names[0]} and {names[1]} is required")
        return [self._opt(what, n, o, (k, _abi.NJ, _abi.NJ)) for n, o in zip(names, outs)]

    def inverse_dynamics_derivatives(self, dtau_dq=None, dtau_dqd=None, qdd=None, env_ids=None, q=None, qd=None, gravity=True):
        """The derivatives of inverse_dynamics at fixed qdd into `dtau_dq` and / or `dtau_dqd`, each (k, 26, 26) f32 and
        derivative-major: out[i, c, r] = d tau_r / d (q or qd)_c (the transpose of the Jacobian).  Either may be None, not both.
        qdd and rows as for inverse_dynamics.  dexsim_inverse_dynamics_derivatives."""
        what = "inverse_dynamics_derivatives"
        ids, qp, vp, k = self._kin_rows_qd(what, env_ids, q, qd)
        ap = self._opt(what, "qdd", qdd, (k, _abi.NJ))
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
        tp = self._opt(what, "tau", tau, (k, _abi.NJ))
        op = self._req(what, "qdd", qdd, (k, _abi.NJ))
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
        tp = self._req("solve_ik", "targets", targets, (k, _abi.NFINGER, 3))
        cp = self._req("solve_ik", "controls", controls, (k, _abi.NACT))
        qo = self._opt("solve_ik", "q_out", q_out, (k, _abi.NJ))
        rp = self._opt("solve_ik", "residual", residual, (k, _abi.NFINGER))
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
        bp = self._opt("proximity", "box_pose", box_pose, (k, 7))
        cp = self._opt("proximity", "cap_env", cap_env, (k, _abi.NCAP, 2, 8))
        sp = self._opt("proximity", "self_min", self_min, (k, _abi.NPROX_GROUPS, 8))
        pp = self._opt("proximity", "pair_dist", pair_dist, (k, _abi.NPROX_PAIRS))
        self._keep_prox = box_pose                  # alive until the kernel ran
        check(self.lib.dexsim_query_proximity(self.h, ids, k, qp, bp, float(box_size), cp, sp, pp, self._stream()), "query_proximity")

    # ------------------------------------------------------------------ range sensors (dexsim_raycast)
    def raycast(self, dist=None, hits=None, rays=None, parent=None, env_ids=None, q=None, box_pose=None, box_size=0.0, min_range=0.0,
                max_range=1.0, skip_parent=False):
        """Cast the rays `rays` (R, 6) f32 on this device -- origin and direction in the parent frame, shared by all rows -- against
        the ground, the box and the hand's capsules in one launch: `dist` (k, R) f32 = metres along the unit direction, +inf without
        a hit; `hits` (k, R, 8) f32 = t, hit point (3), outward unit normal (3), segment id as int32 bits.  Either may be None, not
        both.  parent: a host sequence of R ints, -1 = the env's world frame or a joint index, non-decreasing.  A hit counts inside
        [min_range, max_range]; skip_parent: a ray on joint frame j does not test the capsules that ride on j.  Rows and the box as
        for proximity.  dexsim_raycast."""
        what = "raycast"
        if dist is None and hits is None:
            raise DexSimError(f"{what}: at least one of dist and hits is required")
        if rays is None or parent is None:
            raise DexSimError(f"{what}: rays and parent are required")
        pl = [int(p) for p in parent]
        R = len(pl)
        if not 1 <= R <= _abi.RAY_MAX:
            raise DexSimError(f"{what}: between 1 and {_abi.RAY_MAX} rays, got {R}")
        ids, qp, k = self._kin_rows(what, env_ids, q)
        rp = self._req(what, "rays", rays, (R, 6))
        bp = self._opt(what, "box_pose", box_pose, (k, 7))
        dp = self._opt(what, "dist", dist, (k, R))
        hp = self._opt(what, "hits", hits, (k, R, 8))
        self._keep_ray = (rays, box_pose)            # alive until the kernel ran
        check(self.lib.dexsim_raycast(self.h, ids, k, qp, bp, float(box_size), rp, (C.c_int * R)(*pl), R, float(min_range), float(max_range),
                                      _abi.RAY_SKIP_PARENT if skip_parent else 0, dp, hp, self._stream()), what)


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


class RayHits:
    """What DexHandEnv.read_ray_sensor returns: `dist` (k, R) and `hits` (k, R, 8) device tensors (None where not requested) and views
    of the hit records."""

    def __init__(self, model, dist=None, hits=None):
        self.dist, self.hits = dist, hits
        self._model = model

    @property
    def seg(self):
        """(k, R) int32 segment ids: SEG_NONE, SEG_GROUND, SEG_BOX or SEG_CAPSULE0 + c (word 7 of hits)."""
        return self.hits[..., 7].contiguous().view(torch.int32)

    @property
    def points(self):
        """(k, R, 3) hit points in the env's world frame (zeros without a hit)."""
        return self.hits[..., 1:4]

    @property
    def normals(self):
        """(k, R, 3) outward unit normals at the hit, world frame (zeros without a hit)."""
        return self.hits[..., 4:7]

    def segment_name(self, seg_id):
        """"none", "ground", "box", or the name of the rigid body the hit capsule belongs to (a row name of rigid_body_states)."""
        i = int(seg_id)
        if i in (_abi.SEG_NONE, _abi.SEG_GROUND, _abi.SEG_BOX):
            return ("none", "ground", "box")[i]
        return ProximityResult.capsule_body(self, i - _abi.SEG_CAPSULE0)


class EnvQueries:
    """The user level of the queries.  DexHandEnv supplies _core, _sim_cfg, _model_struct, model, num_envs, actions,
    action_processor and the _cameras and _ray_sensors dicts."""

    # ------------------------------------------------------------------ the argument rules
    def _query_core(self, what, methods, error=NotImplementedError):
        """The core, which must be the HIP engine: a core injected for a test may lack the `methods` of the ctypes level."""
        core = self._core
        for m in methods:
            if not hasattr(core, m):
                raise error(f"{what} needs the HIP engine (DexSimCore): the injected core {type(core).__name__} has no {m}()")
        return core

    @staticmethod
    def _outputs(what, outputs, names):
        """The `outputs` of a query that returns a choice of tensors: one name or several, as a tuple of names from `names`."""
        outputs = (outputs,) if isinstance(outputs, str) else tuple(outputs)
        if not outputs or any(o not in names for o in outputs):
            raise ValueError(f"{what}: outputs must be a non-empty subset of {names}, got {outputs}")
        return outputs

    @staticmethod
    def _box_args(what, box_pose, box_size, k, device):
        """(box_pose as a contiguous (k, 7) float32 device tensor or None, box_size as the float the core takes: 0.0 = the
        configured edge length) of a geometric query."""
        if box_pose is not None:
            box_pose = torch.as_tensor(box_pose, dtype=torch.float32, device=device)
            if tuple(box_pose.shape) != (k, 7):
                raise ValueError(f"{what}: box_pose must have shape ({k}, 7), got {tuple(box_pose.shape)}")
            box_pose = box_pose.contiguous()
        size = 0.0
        if box_size is not None:
            size = float(box_size)
            if not (size > 0.0 and size != float("inf")):
                raise ValueError(f"{what}: box_size must be a positive finite edge length, got {box_size}")
        return box_pose, size

    def _out_buffers(self, what, outputs, shapes, out, ids, device):
        """{name: tensor of shapes[name]} for the names in `outputs`: the caller's tensor where the dict `out` has one, else a new
        one.  With an id list a row whose id is out of range is left as it is by the kernel: a new tensor gets a defined value, NaN."""
        if out is not None and (not isinstance(out, dict) or any(o not in outputs for o in out)):
            raise ValueError(f"{what}: out must be a dict of tensors keyed by the names in outputs, got {out if not isinstance(out, dict) else sorted(out)}")
        bufs = {}
        for o in outputs:
            given = None if out is None else out.get(o)
            bufs[o] = self._kindyn_out(what, given, shapes[o], device)
            if given is None and ids is not None:
                bufs[o].fill_(float("nan"))
        return bufs

    # ------------------------------------------------------------------ save / restore / fork (dexsim_save_state and friends)
    def _state_core(self, what):
        return self._query_core(what, ("state_layout", "state_bank", "save_state", "load_state", "copy_envs", "get_step_stamp",
                                       "set_step_stamp"), DexSimError)

    def _config_hash(self):
        return hashlib.sha256(bytes(self._sim_cfg) + bytes(self._model_struct)).hexdigest()

    def get_state(self):
        """Full snapshot (EnvState) of this env at a control-step boundary; set_state() of it, here or in a fresh env of the
        same configuration, continues bit for bit."""
        core = self._state_core("get_state")
        bank = core.state_bank(core.NS)
        core.save_state(bank)
        ap = self.action_processor
        from .env import EnvState      # (env.py imports this module)
        return EnvState(bank.version, bank.record_words, self.num_envs, self._config_hash(), bank.capacity, core.get_step_stamp(),
                        bank.data, core.stats.clone(), core.counters.clone(), self.actions.clone(),
                        ap._enabled_post_action_filters)

    def set_state(self, state):
        """Restore a snapshot taken by get_state().  Every env-owned tensor (obs_buf, rew_buf, reset_buf, extras, obs_dict,
        dof_state, actor_root_state_tensor, ...) is written in place: the views callers hold stay valid."""
        core = self._state_core("set_state")
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
        src, dst = env_id_vector(src_ids, core.device), env_id_vector(dst_ids, core.device)
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
        core = self._query_core("create_camera", ("render",))
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
        core = self._query_core("render_camera", ("render",))
        c = self._camera(name)
        outputs = tuple(outputs)
        if not outputs or any(o not in ("rgba", "depth", "seg") for o in outputs):
            raise ValueError(f"render_camera: outputs must be a non-empty subset of ('rgba', 'depth', 'seg'), got {outputs}")
        ids = None if env_ids is None else env_id_vector(env_ids, core.device)
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
        core = self._query_core(what, (method,))
        if q is not None:
            q = torch.as_tensor(q, dtype=torch.float32, device=core.device)
            if q.dim() != 2 or q.shape[1] != _abi.NJ or q.shape[0] < 1:
                raise ValueError(f"{what}: q must have shape (k, {_abi.NJ}) with k >= 1, got {tuple(q.shape)}")
            return core, None, q.contiguous(), int(q.shape[0])
        if env_ids is None:
            return core, None, None, self.num_envs
        ids = env_id_vector(env_ids, core.device)
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

    # ------------------------------------------------------------------ forward kinematics
    SITE_SELECTIONS = {"all": slice(0, _abi.NSITE), "base": slice(0, 1), "tips": slice(1, 1 + _abi.NFINGER),
                       "pads": slice(1 + _abi.NFINGER, _abi.NSITE)}

    def _fk_rows(self, what, env_ids, q, qd=None):
        """_kindyn_rows for the forward kinematics: a `qd` override is optional with a `q` override and an error without one."""
        if qd is not None and q is None:
            raise ValueError(f"{what}: a qd override needs a q override (without q the velocities are the envs' own)")
        core, ids, q, k = self._kindyn_rows(what, "forward_kinematics", env_ids, q)
        return core, ids, q, self._kindyn_vel(what, "qd", qd, k, core.device), k

    def _fk_out(self, what, out, shape, core, ids):
        given = out
        out = self._kindyn_out(what, out, shape, core.device)
        if given is None and ids is not None:   # a row whose id is out of range is left as it is by the kernel: give it a defined value
            out.fill_(float("nan"))
        return out

    def get_body_states(self, bodies=None, env_ids=None, q=None, qd=None, out=None):
        """gym.refresh_rigid_body_state_tensor on a row and body selection: (k, nb, 13) rows of rigid_body_states -- position of
        the body-frame origin, quaternion xyzw, world linear and angular velocity -- of the hand bodies `bodies` (as for
        get_jacobian: indices or names, None = all 37 in order).  Rows: the envs `env_ids` (None = all) at their dof_pos / dof_vel,
        or the rows of a (k, 26) joint-position override `q` (env_ids is then ignored) with the optional (k, 26) velocity override
        `qd`; without `qd` the velocity words of an override are exactly zero."""
        what = "get_body_states"
        core, ids, q, qd, k = self._fk_rows(what, env_ids, q, qd)
        idx, nb = self._kindyn_bodies(what, bodies)
        out = self._fk_out(what, out, (k, nb, 13), core, ids)
        core.forward_kinematics(body_states=out, env_ids=ids, q=q, qd=qd, bodies=idx)
        return out

    def get_site_poses(self, sites="all", frame="world", env_ids=None, q=None, out=None):
        """(k, ns, 7) poses (position, quaternion xyzw) of the hand's sites: sites="all" (11: right_hand_base, five tips, five
        pads), "base" (1), "tips" (5) or "pads" (5), thumb to pinky.  frame="world": the env's world frame, as
        obs_dict["fingertip_poses_world"]; frame="hand": relative to right_hand_base, as fingertip_poses_hand /
        fingerpad_poses_hand.  Rows as for get_jacobian.  All 11 are computed into one (k, 11, 7) tensor -- `out`, when given --
        and the selection is a slice of it."""
        what = "get_site_poses"
        if sites not in self.SITE_SELECTIONS:
            raise ValueError(f"{what}: sites must be one of {sorted(self.SITE_SELECTIONS)}, got {sites!r}")
        if frame not in ("world", "hand"):
            raise ValueError(f"{what}: frame must be 'world' or 'hand', got {frame!r}")
        core, ids, q, _, k = self._fk_rows(what, env_ids, q)
        out = self._fk_out(what, out, (k, _abi.NSITE, 7), core, ids)
        core.forward_kinematics(site_poses=out, env_ids=ids, q=q, hand_frame=frame == "hand")
        return out[:, self.SITE_SELECTIONS[sites]]

    def get_centroid(self, env_ids=None, q=None, qd=None, out=None):
        """The hand as one body: a dict of views of one (k, 8) tensor (`out`, when given) -- "com" (k, 3) centre of mass in the
        world frame, "com_vel" (k, 3) its velocity, "kinetic" (k,) = 1/2 qd^T M(q) qd with the M of get_mass_matrix, "potential"
        (k,) = -M_tot g . com (zero at the env's world origin) -- plus "data", the tensor itself.  Rows and overrides as for
        get_body_states; without velocities com_vel and kinetic are exactly zero."""
        what = "get_centroid"
        core, ids, q, qd, k = self._fk_rows(what, env_ids, q, qd)
        out = self._fk_out(what, out, (k, 8), core, ids)
        core.forward_kinematics(centroid=out, env_ids=ids, q=q, qd=qd)
        return {"com": out[:, 0:3], "potential": out[:, 3], "com_vel": out[:, 4:7], "kinetic": out[:, 7], "data": out}

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
        outputs = self._outputs(what, outputs, ("cap_env", "self_min", "pair_dist"))
        if isinstance(box_pose, str):
            if box_pose != "env":
                raise ValueError(f"{what}: box_pose must be a (k, 7) tensor, 'env' or None, got {box_pose!r}")
            if q is None or k != self.num_envs:
                raise ValueError(f"{what}: box_pose='env' needs a q override of num_envs = {self.num_envs} rows")
            if not int(self._sim_cfg.has_box):
                raise ValueError(f"{what}: box_pose='env' needs a task with a box")
            box_pose = core.root_state[:, 1, :7]
        box_pose, size = self._box_args(what, box_pose, box_size, k, core.device)
        shapes = {"cap_env": (k, _abi.NCAP, 2, 8), "self_min": (k, _abi.NPROX_GROUPS, 8), "pair_dist": (k, _abi.NPROX_PAIRS)}
        bufs = self._out_buffers(what, outputs, shapes, out, ids, core.device)
        core.proximity(env_ids=ids, q=q, box_pose=box_pose, box_size=size, **bufs)
        if getattr(self, "_proximity_pairs", None) is None:
            self._proximity_pairs = core.proximity_pairs()                     # a host table: read once
        return ProximityResult(self.model, self._proximity_pairs, **bufs)

    # ------------------------------------------------------------------ range sensors (dexsim_raycast)
    def _ray_parent(self, what, p):
        """(joint index or -1, body index or None) of one `parent` entry: None = the world frame, a joint index, a DOF name or a body
        name of hand_model.BODY_NAMES."""
        if p is None:
            return -1, None
        if isinstance(p, str):
            if p in self.model.dof_names:
                return self.model.dof_names.index(p), None
            if p in self.model.body_names:
                b = self.model.body_names.index(p)
                return int(self.model.body_parent[b]), b
            raise ValueError(f"{what}: unknown parent '{p}' (a joint of {self.model.dof_names} or a body of {self.model.body_names})")
        j = int(p)
        if not 0 <= j < _abi.NJ:
            raise ValueError(f"{what}: a parent joint index must be in [0, {_abi.NJ}), got {p}")
        return j, None

    def create_ray_sensor(self, name, origins, directions, parent=None, min_range=0.0, max_range=1.0, skip_parent=False):
        """A range sensor of R rays for every env: origins and directions (R, 3) in each ray's parent frame.  parent: one value
        or R of them -- None = the env's world frame, a joint index or DOF name = that joint's frame (as create_camera), or a body
        name from hand_model.BODY_NAMES such as "r_f_link2_pad": the ray is then given in the body's frame and folded, on the host and
        in float64, through the body's fixed offset into the joint frame the body rides on (a body on the spawn frame folds to the
        world frame).  A reading counts inside [min_range, max_range] metres; skip_parent: a ray does not see the capsules of the
        joint frame it is mounted on (a sensor under its own link's skin).  The device call wants the rays sorted by parent: they are
        sorted here, stably.  If the given order was already sorted, read_ray_sensor returns the kernel's tensors as they are;
        otherwise every read puts the columns back into the caller's order by one index_select (a copy)."""
        what = "create_ray_sensor"
        core = self._query_core(what, ("raycast",))
        sensors = self._ray_sensors
        if name in sensors:
            raise ValueError(f"{what}: ray sensor '{name}' already exists")
        o, d = np.asarray(origins, dtype=np.float64), np.asarray(directions, dtype=np.float64)
        if o.ndim != 2 or o.shape[1] != 3 or d.shape != o.shape:
            raise ValueError(f"{what}: origins and directions must both have shape (R, 3), got {o.shape} and {d.shape}")
        R = o.shape[0]
        if not 1 <= R <= _abi.RAY_MAX:
            raise ValueError(f"{what}: between 1 and {_abi.RAY_MAX} rays, got {R}")
        if not (np.isfinite(o).all() and np.isfinite(d).all()) or ((d * d).sum(1) < 1e-24).any():
            raise ValueError(f"{what}: origins and directions must be finite and no direction may be zero")
        lo, hi = float(min_range), float(max_range)
        if not (np.isfinite(lo) and np.isfinite(hi) and 0.0 <= lo < hi):
            raise ValueError(f"{what}: the ranges must be finite with 0 <= min_range < max_range, got {min_range} and {max_range}")
        plist = list(parent) if isinstance(parent, (list, tuple, np.ndarray)) else [parent] * R
        if len(plist) != R:
            raise ValueError(f"{what}: parent must be one value or {R} of them, got {len(plist)}")
        o, d = o.copy(), d.copy()                                              # directions as given: the device call normalises them
        joints = np.zeros(R, dtype=np.int64)
        for i, p in enumerate(plist):
            joints[i], b = self._ray_parent(what, p)
            if b is not None:                                                   # body frame -> the frame the body rides on
                Rb, pb = np.asarray(self.model.body_R[b], dtype=np.float64), np.asarray(self.model.body_p[b], dtype=np.float64)
                o[i], d[i] = pb + Rb @ o[i], Rb @ d[i]
                if joints[i] < 0:                                               # a body on the spawn frame: the world frame, through the spawn pose
                    Rs = np.asarray(self.model.spawn_rot, dtype=np.float64)
                    o[i], d[i] = np.asarray(self.model.spawn_pos, dtype=np.float64) + Rs @ o[i], Rs @ d[i]
        order = np.argsort(joints, kind="stable")
        rays = torch.as_tensor(np.concatenate([o, d], axis=1)[order], dtype=torch.float32).to(core.device).contiguous()
        unsort = None
        if (order != np.arange(R)).any():
            unsort = torch.as_tensor(np.argsort(order, kind="stable"), dtype=torch.int64).to(core.device)
        sensors[name] = {"rays": rays, "parent": [int(j) for j in joints[order]], "unsort": unsort, "min_range": lo, "max_range": hi,
                         "skip_parent": bool(skip_parent), "R": R}
        return name

    def read_ray_sensor(self, name, env_ids=None, q=None, box_pose=None, box_size=None, outputs=("dist",), out=None):
        """Read the ray sensor `name`, one kernel launch: a RayHits with `dist` (k, R) -- metres along the ray, +inf without a hit
        -- and / or `hits` (k, R, 8) -- t, hit point (3), outward unit normal (3), segment id as int32 bits; its views seg, points
        and normals, and segment_name(id).  Point and normal are in the env's world frame.  Rows as for get_jacobian: the envs
        `env_ids` (None = all), or the rows of a (k, 26) joint-position override `q`.  The box: `box_pose` (k, 7) = centre xyz +
        quaternion xyzw when given; None = the envs' own box without `q`, no box with it.  box_size: edge length, None = the
        configured one.  out: a dict of preallocated tensors by output name; with a sensor whose rays were given out of parent order
        the reordered copy is what is returned, and `out` receives the kernel's own order."""
        what = "read_ray_sensor"
        core, ids, q, k = self._kindyn_rows(what, "raycast", env_ids, q)
        sensors = self._ray_sensors
        if name not in sensors:
            raise KeyError(f"no ray sensor named '{name}' (ray sensors: {sorted(sensors)})")
        s = sensors[name]
        outputs = self._outputs(what, outputs, ("dist", "hits"))
        box_pose, size = self._box_args(what, box_pose, box_size, k, core.device)
        bufs = self._out_buffers(what, outputs, {"dist": (k, s["R"]), "hits": (k, s["R"], 8)}, out, ids, core.device)
        core.raycast(rays=s["rays"], parent=s["parent"], env_ids=ids, q=q, box_pose=box_pose, box_size=size, min_range=s["min_range"],
                     max_range=s["max_range"], skip_parent=s["skip_parent"], **bufs)
        if s["unsort"] is not None:
            bufs = {o: t.index_select(1, s["unsort"]) for o, t in bufs.items()}
        return RayHits(self.model, **bufs)
