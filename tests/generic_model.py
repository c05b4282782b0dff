"""One hand model with none of the default model's exact zeros, ones and repeated numbers, for the rigs (tests/query_rig.py,
tests/physics_rig.py).  A plain module: no fixtures, imported by the rigs and by no test module but its own.

The default HandModel -- and every copy of it that only MULTIPLIES its numbers -- has identity joint offsets on 21 joints, zero base
offsets (the origins of joints 3, 4, 5 coincide), unit axes along e_x / e_y / e_z, offsets and centres of mass on the x axis, a
diagonal palm inertia, identity site and body frames, capsules from the joint origin along x, and the same gains, armature and link
masses on every finger.  A kernel that takes a lever about the wrong one of three coincident origins, composes an offset on the wrong
side, drops a y or z component or reads a neighbour's constant gives the right answer on such a model.

generic(hand, seed) edits a HandModel within what validate_model (csrc/dexsim.hip) demands -- joint types, massless links 0-4,
capsule, site and body parents -- by tenths of a radian and about a centimetre: large against every bound of the suites (1e-5 m, 1e-5
per rotation entry), small enough that the hand stays a hand.  Every number it writes is a float32, so the model is the same one
after export_mjcf / load_mjcf (tests/test_generic_model.py).  The palm, pad and tip bodies stay tied to their sites and the link
bodies welded to their joint frames, as the MJCF dialect has them; free_body_frames(ms, seed) gives all 37 bodies frames of their own
in the struct, which is what the queries read.

RESTORE names each property of the list above with a function that puts it back to the default's value on a generic model: the
bite test builds those models and shows that every property moves a float64 reference by at least 10 bounds.
"""
import copy
import functools

import numpy as np

from dexrobot_isaac_amd import _abi
from dexrobot_isaac_amd.config import build_sim_config, default_cfg
from dexrobot_isaac_amd.hand_model import HandModel, mat_to_quat_xyzw, quat_xyzw_to_mat

NJ, NB, NS, NCAP = _abi.NJ, _abi.NUM_HAND_BODIES, _abi.NSITE, _abi.NCAP
# The model's seed.  Seeds 1-7 were drawn and looked at from the references alone (never from a device result).  On seeds 2, 3, 5, 6
# and 7 a condition that a suite sets for ITS OWN reference fails, each by little: the fp32 oracle's gravity-force roundoff on 300 poses
# exceeds test_kindyn's cap (4 e_g = 1.07e-5 > 1e-5), the float64 IK reference converges on fewer than 90 % of the rows (80-89 %), its
# float32 evaluation leaves more than test_ik's floor (1.75e-6 m > 1.4e-6 m), or the float32 centre of mass of the FK reference is off
# by more than a tenth of its bound (1.03e-6 m, the hand 2.5 m from the origin).  Seeds 1 and 4 meet all of them; 4 has the wider
# margin on e_g (4 e_g = 8.2e-6; seed 1: 9.6e-6).
SEED = 4
FLEXION = [6 + 4 * f + l for f in range(5) for l in (1, 2, 3)]
FINGER_JOINTS = list(range(6, NJ))
MASSIVE = list(range(5, NJ))


def f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def rotation(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def _signed(rng, lo, hi, size=None):
    """Uniform in [lo, hi] with a random sign: never near zero."""
    return rng.choice([-1.0, 1.0], size) * rng.uniform(lo, hi, size)


def _push(rng, v, lo, hi):
    """v moved by lo..hi per component, away from zero where a component has a sign (so that none ends up near zero)."""
    v = np.asarray(v, dtype=np.float64)
    return v + np.where(v == 0, rng.choice([-1.0, 1.0], v.shape), np.sign(v)) * rng.uniform(lo, hi, v.shape)


def _skew_axis(rng):
    """A unit vector whose three components are all at least 0.25 in size."""
    a = _signed(rng, 0.4, 1.0, 3)
    return a / np.linalg.norm(a)


def _turn(rng, lo, hi):
    return rotation(_skew_axis(rng), rng.uniform(lo, hi))


UNIT = 4e-9        # a float32 axis or quaternion of the model is a unit vector to this (a float32 vector is to 6e-8 in general)


def _turned(rng, R0, lo, hi):
    """R0 turned by lo..hi rad about a skew axis, as the rotation of a float32 quaternion -- what the struct and an MJCF file hold --
    drawn again until that quaternion is a unit vector to UNIT: the references normalise the model's quaternions and the engine
    and the oracle do not (tests/dynderiv_ref.py::frames), which is not what this model is about."""
    while True:
        q = f32(mat_to_quat_xyzw(R0 @ _turn(rng, lo, hi)))
        if abs(np.linalg.norm(q) - 1) <= UNIT:
            return quat_xyzw_to_mat(q)


def _tilted(rng, a0):
    """The axis a0 with 0.1-0.35 added to each of its zero components, renormalised, as float32 numbers; unit to UNIT."""
    while True:
        a = a0 + np.where(a0 == 0, _signed(rng, 0.1, 0.35, 3), 0.0)
        a = f32(a / np.linalg.norm(a))
        if abs(np.linalg.norm(a) - 1) <= UNIT:
            return a


def _sym(s):
    return np.array([[s[0], s[3], s[4]], [s[3], s[1], s[5]], [s[4], s[5], s[2]]])


def _sym6(I):
    return [I[0, 0], I[1, 1], I[2, 2], I[0, 1], I[0, 2], I[1, 2]]


def tie_bodies(hand):
    """The palm, pad and tip bodies on their sites, the link bodies on their joint frames: load_mjcf's rule."""
    hand.body_R, hand.body_p = np.tile(np.eye(3), (NB, 1, 1)), np.zeros((NB, 3))
    hand.body_R[6], hand.body_p[6] = hand.site_R[0], hand.site_p[0]
    for f in range(5):
        b0 = 7 + 6 * f
        hand.body_R[b0 + 4], hand.body_p[b0 + 4] = hand.site_R[6 + f], hand.site_p[6 + f]
        hand.body_R[b0 + 5], hand.body_p[b0 + 5] = hand.site_R[1 + f], hand.site_p[1 + f]


def generic(hand: HandModel, seed=SEED) -> None:
    """Edit `hand` in place (module docstring).  Magnitudes: joint and site frames turned by 0.2-0.5 rad about a skew axis, offsets
    moved by 4-12 mm per component, axes tilted by 0.1-0.35 per component and renormalised, centres of mass moved by 2-5 mm per
    component, inertia tensors turned by 0.3-1.2 rad, gains and masses varied by up to +-30 % per joint, armatures 0.5-2 e-4, limits
    moved by up to 0.05 rad (the lower finger limits downwards, so that q = 0 stays in range), the spawn frame turned by 0.5-1 rad."""
    rng = np.random.default_rng(seed)
    hand.spawn_rot = _turned(rng, hand.spawn_rot, 0.5, 1.0)
    for j in range(NJ):
        hand.jRoff[j] = _turned(rng, hand.jRoff[j], 0.2, 0.5)
        hand.jpoff[j] = _push(rng, hand.jpoff[j], 4e-3, 12e-3)
        hand.jaxis[j] = _tilted(rng, hand.jaxis[j])
        hand.kp[j] *= rng.uniform(0.7, 1.3)
        hand.kd[j] *= rng.uniform(0.7, 1.3)
        hand.armature[j] = rng.uniform(0.5e-4, 2e-4)
        down = rng.uniform(0.005, 0.05)
        hand.lo[j] += -down if j >= 6 else _signed(rng, 0.005, 0.05)
        hand.hi[j] += _signed(rng, 0.005, 0.05)
    for j in MASSIVE:
        hand.mass[j] *= rng.uniform(0.7, 1.3)
        hand.com[j] = _push(rng, hand.com[j], 2e-3, 5e-3)
        while True:                                                  # the physical tensor in a turned frame: no entry is invented
            R = _turn(rng, 0.3, 1.2)
            I = R @ _sym(hand.inertia[j]) @ R.T
            if np.abs([I[0, 1], I[0, 2], I[1, 2]]).min() >= 0.02 * np.abs(np.diag(I)).max():
                break
        hand.inertia[j] = _sym6(I)
    for s in range(NS):
        hand.site_R[s] = _turned(rng, hand.site_R[s], 0.2, 0.5)
        hand.site_p[s] = _push(rng, hand.site_p[s], 2e-3, 8e-3)
    for c in range(NCAP):
        hand.cap_p0[c] = _push(rng, hand.cap_p0[c], 2e-3, 5e-3)
        hand.cap_p1[c] = _push(rng, hand.cap_p1[c], 2e-3, 5e-3)
    for name in ("jpoff", "jaxis", "kp", "kd", "armature", "lo", "hi", "mass", "com", "inertia", "site_p", "cap_p0", "cap_p1"):
        setattr(hand, name, f32(getattr(hand, name)))
    assert (hand.hi > hand.lo).all()
    tie_bodies(hand)


def free_body_frames(ms, seed=SEED) -> None:
    """Frames of their own for all 37 bodies, in the struct (the MJCF dialect cannot say them): body_q a turn of 0.2-1 rad about a
    skew axis, body_p 2-10 mm per component.  body_parent stays."""
    rng = np.random.default_rng(seed + 1000)
    for b in range(NB):
        q = mat_to_quat_xyzw(_turned(rng, np.eye(3), 0.2, 1.0))
        p = _signed(rng, 2e-3, 10e-3, 3)
        for i in range(4):
            ms.body_q[b][i] = float(q[i])
        for i in range(3):
            ms.body_p[b][i] = float(p[i])


# ------------------------------------------------------------------------------------------------- one property put back
def _default_like(hand):
    return HandModel(hand.spawn_pos, (0.0, 0.0, 0.0, 1.0))


def _restore(names, rows=None):
    def fn(hand):
        d = _default_like(hand)
        for n in names:
            if rows is None:
                setattr(hand, n, getattr(d, n).copy())
            else:
                getattr(hand, n)[rows] = getattr(d, n)[rows]
        tie_bodies(hand)
    return fn


def _uniform(name):
    """The fingers' numbers the same on every finger again: finger f's link l takes the index finger's (the thumb's masses keep
    their factor 1.2, as the default has it -- what matters is that l is no longer visible within a finger group)."""
    def fn(hand):
        a = getattr(hand, name)
        for f in range(5):
            for l in range(4):
                a[6 + 4 * f + l] = a[6 + 4 * 1] if name != "mass" else a[6 + 4 * 1 + l]
    return fn


def _zero_yz(name, rows):
    def fn(hand):
        getattr(hand, name)[rows, 1:] = 0.0
    return fn


def _palm_diagonal(hand):
    hand.inertia[5, 3:] = 0.0


def _cap_p1_on_x(hand):
    hand.cap_p1[3:, 1:] = 0.0


RESTORE = {
    "spawn identity": _restore(["spawn_rot"]),
    "base jqoff identity": _restore(["jRoff"], list(range(6))),
    "base jpoff zero": _restore(["jpoff"], list(range(6))),
    "base axes e_x e_y e_z": _restore(["jaxis"], list(range(6))),
    "flexion jqoff identity": _restore(["jRoff"], FLEXION),
    "flexion axes -e_y": _restore(["jaxis"], FLEXION),
    "flexion jpoff y, z zero": _zero_yz("jpoff", FLEXION),
    "finger com y, z zero": _zero_yz("com", FINGER_JOINTS),
    "palm products of inertia zero": _palm_diagonal,
    "site_q identity on tips and pads": _restore(["site_R"], list(range(1, NS))),
    "site 0 on the palm joint's origin": _restore(["site_R", "site_p"], [0]),
    "cap_p0 zero on the fingers": _restore(["cap_p0"], list(range(3, NCAP))),
    "cap_p1 on the x axis": _cap_p1_on_x,
    "kp uniform": _uniform("kp"),
    "kd uniform": _uniform("kd"),
    "armature zero": _restore(["armature"]),
    "mass uniform": _uniform("mass"),
    "body_q, body_p default": None,                                   # the struct edit left out (build's free_bodies)
}


# ------------------------------------------------------------------------------------------------- the cached builder
@functools.lru_cache(maxsize=None)
def _built(n, task, seed, restore):
    cfg = default_cfg(task)
    cfg["env"]["numEnvs"] = n
    hand = HandModel(cfg["env"]["initialHandPos"], cfg["env"]["initialHandRot"])
    generic(hand, seed)
    if restore is not None and RESTORE[restore] is not None:
        RESTORE[restore](hand)
    sc, hand = build_sim_config(cfg, model=hand)
    return sc, hand


def build(n, task="BlindGrasping", seed=SEED, free_bodies=False, restore=None):
    """(sc, model, ms) of n envs on the generic model, the configuration and the HandModel built once per process; the struct is a
    fresh one on every call (the suites edit theirs).  free_bodies: free_body_frames on the struct.  restore: a name of RESTORE."""
    sc, hand = _built(n, task, seed, restore)
    ms = hand.to_struct()
    if free_bodies and restore != "body_q, body_p default":
        free_body_frames(ms, seed)
    return sc, copy.deepcopy(hand), ms
