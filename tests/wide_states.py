"""Seeded contact-free states over the hand's WHOLE joint range for the physics parity tests (tests/test_wide_poses.py).  Plain numpy.

physics_rig.random_state, and tests/tumbled_states.py on top of it, draw finger joints from [0, 0.5] rad, base rotations from
+-0.3 rad and joint speeds from N(0, 0.3), clipped to at least 1 mm / 1 mrad inside every limit: the velocity terms of the bias force
are worth a few bounds there, no half-angle leaves quadrant 0 of sincos_joint, and no joint reaches a stop.  Here (h = dt / substeps):
  fingers        q ~ U(lo, hi) per joint, qd ~ N(0, 3), target q + N(0, 0.05)
  base slides    x, y ~ U(-0.15, 0.15), z ~ U(0, 0.2) (the hand is >= 0.3 m above box and ground in any orientation), qd ~ N(0, 0.5)
  base rotations q ~ U(-3, 3), qd ~ N(0, 2)
  base targets   q + h qd + N(0, 0.002): the base drives are implicit PD with k_p = 1e4, a target 0.3 rad away snaps the joint
                 there at over 100 rad/s, a regime of no interest
  box            upright at rest at the origin, z = box_size / 2: there only so that the BlindGrasping kernels run
Kind "free" is that draw.  Kind "stops" is the same draw with, in the odd envs, each finger joint with probability 0.4 put at
U(0, 3 h) rad inside one of its limits (either, with equal probability), moving into it at 2-6 rad/s, its target 0.2 rad beyond the
stop: after one sub-step the joint is on the stop, and it is driven into it again in every sub-step that follows.

Every array is [rows][n] float64 holding float32-representable numbers, as in tests/tumbled_states.py: the fp64 oracle, the fp32
oracle and the kernels start from the very same state.  The limits are the float32 ones of the model struct, which is what all
three clamp at.
"""
import functools

import numpy as np

from tests.tumbled_states import f32

P_STOP, STOP_BAND, STOP_SPEED, STOP_TARGET = 0.4, 3.0, (2.0, 6.0), 0.2


def limits(ms):
    """(lo, hi) of the model struct: the float32 numbers the oracles and the kernels clamp at, as float64 arrays."""
    return (np.array(np.ctypeslib.as_array(ms.lo), dtype=np.float64), np.array(np.ctypeslib.as_array(ms.hi), dtype=np.float64))


def _draw(kind, n, seed, sc, model):
    assert kind in ("free", "stops")
    rng = np.random.default_rng(seed)
    lo, hi = limits(model.to_struct())
    h = float(sc.dt) / int(sc.substeps)
    q = rng.uniform(lo[:, None], hi[:, None], (26, n))
    q[0:2] = rng.uniform(-0.15, 0.15, (2, n))
    q[2] = rng.uniform(0.0, 0.2, n)
    q[3:6] = rng.uniform(-3.0, 3.0, (3, n))
    qd = rng.normal(0, 3.0, (26, n))
    qd[0:3] = rng.normal(0, 0.5, (3, n))
    qd[3:6] = rng.normal(0, 2.0, (3, n))
    q, qd = f32(q), f32(qd)
    tg = q + rng.normal(0, 0.05, (26, n))
    tg[0:6] = q[0:6] + h * qd[0:6] + rng.normal(0, 0.002, (6, n))
    # the stops: drawn for both kinds, so that "free" and "stops" differ in nothing else
    pick = rng.random((20, n)) < P_STOP
    pick[:, 0::2] = False
    upper = rng.random((20, n)) < 0.5
    depth = rng.uniform(0.0, STOP_BAND * h, (20, n))
    speed = rng.uniform(STOP_SPEED[0], STOP_SPEED[1], (20, n))
    if kind == "stops":
        flo, fhi = lo[6:, None], hi[6:, None]
        q[6:] = np.where(pick, np.where(upper, fhi - depth, flo + depth), q[6:])
        qd[6:] = np.where(pick, np.where(upper, speed, -speed), qd[6:])
        tg[6:] = np.where(pick, np.where(upper, fhi + STOP_TARGET, flo - STOP_TARGET), tg[6:])
        q[6:] = np.clip(f32(q[6:]), flo, fhi)               # rounding to float32 must not put a joint outside its range
    z = np.zeros(n)
    st = dict(q=q, qd=qd, targets=tg, box_pos=np.stack([z, z, z + 0.5 * float(sc.box_size)]), box_quat=np.stack([z, z, z, z + 1.0]),
              box_lin=np.zeros((3, n)), box_ang=np.zeros((3, n)))
    return {k: f32(v) for k, v in st.items()}


@functools.lru_cache(maxsize=None)
def _cached(kind, n, seed):
    from dexrobot_isaac_amd.config import build_sim_config, default_cfg
    cfg = default_cfg("BlindGrasping")
    cfg["env"]["numEnvs"] = n
    return _draw(kind, n, seed, *build_sim_config(cfg))


_BY_CONFIG = {}


def sample(kind, n=256, seed=11, config=None):
    """The "free" / "stops" state of n envs, built once per process; a fresh copy.  `config`: None for the default BlindGrasping
    configuration, or (sc, model) -- a DexSimConfig of n envs and the hand model it goes with (tumbled_states.sample's convention);
    the sample is kept per value of the two structs."""
    if config is None:
        st = _cached(kind, n, seed)
    else:
        sc, model = config
        assert int(sc.num_envs) == n
        key = (kind, n, seed, bytes(sc), bytes(model.to_struct()))
        if key not in _BY_CONFIG:
            _BY_CONFIG[key] = _draw(kind, n, seed, sc, model)
        st = _BY_CONFIG[key]
    return {k: v.copy() for k, v in st.items()}
