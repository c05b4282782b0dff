"""Float64 reference for the kinematics / dynamics tensors (dexsim_body_jacobian, dexsim_mass_matrix) and the error metrics of
tests/test_kindyn.py.

The Jacobian is the textbook geometric one, built from tests/render_ref.HandGeometry.fk (its own forward kinematics from the
header's joint-frame formula) plus body_parent / body_p of the model struct; it shares no code with the engine.  Every function
takes `dtype`, so the SAME code can be evaluated in float32: that difference is the roundoff figure e_J.  M(q) and the gravity
force come from the CPU oracle (oracle/dexsim_oracle.c: crba, and rnea_bias at qd = 0), whose fp32 and fp64 builds give e_M, e_g.
"""
import numpy as np

from dexrobot_isaac_amd import _abi
from oracle.oracle import Oracle
from tests import render_ref as rr

NB, NJ = _abi.NUM_HAND_BODIES, _abi.NJ


class HandKin:
    def __init__(self, ms):
        self.geom = rr.HandGeometry(ms)
        self.body_parent = np.array(np.ctypeslib.as_array(ms.body_parent))
        self.body_p = np.array(np.ctypeslib.as_array(ms.body_p), dtype=np.float64)
        g = self.geom
        self.ancestors = []                                   # joints that move joint frame j, j included
        for j in range(NJ):
            a, p = [], j
            while p >= 0:
                a.append(p)
                p = g.parent(p)
            self.ancestors.append(a)

    def body_frames(self, q, dtype=np.float64):
        """World origins (37, 3) and rotations (37, 3, 3) of the frames the hand bodies are welded to (body_q, a constant
        rotation on top, does not enter a velocity), plus the joint frames."""
        g = self.geom
        o, R = g.fk(q, dtype)
        p = np.zeros((NB, 3), dtype=dtype)
        Rb = np.zeros((NB, 3, 3), dtype=dtype)
        for b in range(NB):
            j = int(self.body_parent[b])
            po, pR = (g.spawn_pos.astype(dtype), rr.quat_to_mat(g.spawn_quat, dtype)) if j < 0 else (o[j], R[j])
            p[b] = po + pR @ self.body_p[b].astype(dtype)
            Rb[b] = pR
        return p, Rb, o, R

    def jacobian(self, q, dtype=np.float64):
        """(37, 6, 26): rows 0-2 world linear velocity of the body origin, rows 3-5 world angular velocity, per unit joint velocity."""
        g = self.geom
        p, _, o, R = self.body_frames(q, dtype)
        J = np.zeros((NB, 6, NJ), dtype=dtype)
        for b in range(NB):
            j = int(self.body_parent[b])
            if j < 0:
                continue
            for c in self.ancestors[j]:
                a = R[c] @ g.jaxis[c].astype(dtype)
                if g.jtype[c] == 0:
                    J[b, 0:3, c] = a
                else:
                    J[b, 0:3, c] = np.cross(a, p[b] - o[c])
                    J[b, 3:6, c] = a
        return J

    def random_poses(self, n, seed):
        """Uniform over the full joint range [lo, hi] (base rotations +-pi included), rounded to float32: what both sides are given."""
        rng = np.random.default_rng(seed)
        g = self.geom
        return rng.uniform(g.lo, g.hi, (n, NJ)).astype(np.float32)


def oracle_pair(sc, ms):
    return Oracle(sc, ms, f64=False), Oracle(sc, ms, f64=True)


def mass_gravity(orc, q):
    """M (n, 26, 26) and the gravity force (n, 26) of the oracle for the poses q (n, 26), as float64 arrays."""
    M = np.zeros((len(q), NJ, NJ))
    g = np.zeros((len(q), NJ))
    zero = np.zeros(NJ)
    for i in range(len(q)):
        M[i], g[i] = orc.mass_matrix(np.asarray(q[i], dtype=np.float64), zero)
    return M, g


def err_M(M, M64):
    """max over poses and i, j of |M - M64|_ij / sqrt(M64_ii M64_jj)."""
    d = np.sqrt(np.einsum("nii->ni", M64))
    return float((np.abs(np.asarray(M, dtype=np.float64) - M64) / (d[:, :, None] * d[:, None, :])).max())


def err_g(g, g64, M64):
    """max_j |g - g64|_j / sqrt(M64_jj), over the max_j |g64|_j / sqrt(M64_jj) of the same pose; the max over poses."""
    d = np.sqrt(np.einsum("nii->ni", M64))
    num = (np.abs(np.asarray(g, dtype=np.float64) - g64) / d).max(1)
    den = (np.abs(g64) / d).max(1)
    return float((num / den).max())


def gpu_mass(core, k, env_ids=None, q=None, mass=True, gravity=True):
    """core.mass_matrix into guarded outputs (tests/query_rig.py): (M, g) as numpy arrays, None for one not asked for."""
    from tests.query_rig import guarded, guards_ok
    fm, M = guarded(k, NJ, NJ) if mass else (None, None)
    fg, g = guarded(k, NJ) if gravity else (None, None)
    core.mass_matrix(mass=M, gravity=g, env_ids=env_ids, q=q)
    for f in (fm, fg):
        if f is not None:
            guards_ok(f)
    return (None if M is None else M.cpu().numpy()), (None if g is None else g.cpu().numpy())
