"""A seeded MIXED contact-rich state for the physics parity tests (tests/test_contact_rich.py).  Plain numpy.

physics_rig.lowered_hand_state draws every env of a test from one regime -- all hands at one height over a box at rest at the origin --
so every lane of a workgroup deals the same kind of work.  Here env i is of class i % 4, so that every workgroup, the padded last one
included, holds every class side by side (N = 134: two full workgroups and one with six live lanes):

  class  hand height q[2]    base rotations   what the contact solver sees
  0      -0.20  +- 0.02      +- 0.1           the hand clear of everything, the box on the ground: box / ground rows only
  1      -0.292 +- 0.004     +- 0.1           8-12 hand contacts: every one a solver block of its own
  2      -0.32  +- 0.004     +- 0.1           mostly more than 12 hand contacts: blocks are pairs
  3      -0.42  +- 0.02      +- 0.15          fingers and palm on box and ground: the list is cut at DEXSIM_KMAX = 24

and beyond lowered_hand_state: finger joints U(0, 0.3) with about 15 % of them put within 8 mrad of their lower stop (joint-limit rows
in the configuration that has them), joint speeds N(0, 0.1), targets q + N(0, 0.02), the box yawed U(-pi, pi) within +-1 cm of the
origin, moving at N(0, 0.03) m/s and N(0, 0.3) rad/s.

Every array is [rows][n] float64 holding float32-representable numbers, as in tests/tumbled_states.py: the fp64 oracle, the fp32
oracle and the kernels start from the very same state.  Quaternions are (x, y, z, w).
"""
import functools

import numpy as np

from tests.tumbled_states import f32

N, SEED = 134, 7
CLASSES = ((-0.20, 0.02, 0.1), (-0.292, 0.004, 0.1), (-0.32, 0.004, 0.1), (-0.42, 0.02, 0.15))     # z, dz, rot of class i % 4
P_STOP, STOP_BAND = 0.15, 8e-3


def _draw(n, seed, lo, box_size):
    rng = np.random.default_rng(seed)
    cls = np.arange(n) % 4
    z, dz, rot = (np.array([c[k] for c in CLASSES])[cls] for k in range(3))
    q = np.zeros((26, n))
    q[2] = z + dz * rng.uniform(-1.0, 1.0, n)
    q[3:6] = rot * rng.uniform(-1.0, 1.0, (3, n))
    q[6:] = rng.uniform(0.0, 0.3, (20, n))
    at_stop = rng.random((20, n)) < P_STOP
    q[6:] = np.where(at_stop, lo[6:, None] + rng.uniform(0.0, STOP_BAND, (20, n)), q[6:])
    q = f32(q)
    q[6:] = np.maximum(q[6:], lo[6:, None])                  # rounding to float32 must not put a joint outside its range
    yaw = rng.uniform(-np.pi, np.pi, n)
    quat = f32(np.stack([0 * yaw, 0 * yaw, np.sin(yaw / 2), np.cos(yaw / 2)]))
    quat = quat / np.linalg.norm(quat, axis=0)               # float32 numbers, unit to float32 roundoff
    st = dict(q=q, qd=rng.normal(0, 0.1, (26, n)), targets=q + rng.normal(0, 0.02, (26, n)),
              box_pos=np.stack([rng.uniform(-0.01, 0.01, n), rng.uniform(-0.01, 0.01, n), np.full(n, 0.5 * box_size + 5e-4)]),
              box_quat=quat, box_lin=rng.normal(0, 0.03, (3, n)), box_ang=rng.normal(0, 0.3, (3, n)))
    return {k: f32(v) for k, v in st.items()}


@functools.lru_cache(maxsize=None)
def _cached(n, seed):
    from dexrobot_isaac_amd.config import build_sim_config, default_cfg
    cfg = default_cfg("BlindGrasping")
    cfg["env"]["numEnvs"] = n
    sc, model = build_sim_config(cfg)
    lo = np.array(np.ctypeslib.as_array(model.to_struct().lo), dtype=np.float64)      # the float32 limits all three clamp at
    return _draw(n, seed, lo, float(sc.box_size))


def sample(n=N, seed=SEED):
    """The mixed state of n envs at the default BlindGrasping model and box (the limit-row configuration shares both), built once per
    process; a fresh copy."""
    return {k: v.copy() for k, v in _cached(n, seed).items()}
