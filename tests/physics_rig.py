"""What the physics parity tests share (test_gpu_parity, test_tumbled_box, test_wide_poses, test_physics_configs, test_model_structure,
test_contact_rich, test_per_env_box):
configurations, the backends loaded with one state, snapshots, the references of the tumbled samples and the comparisons with their
bounds.  A plain module: no fixtures, no torch at import (the HIP backend is imported where one is built).

Bounds.  Integers (list length, type, capsule, corner per slot) are exact over the envs whose list length agrees in the fp64 oracle, the
fp32 oracle and the backend under test; at most LEFT_OUT of the envs may be left out.  Points and gaps: 2e-6 m.  Normals of hand / box
entries: C_RULE E / dist + 1e-7 with E the largest err_n dist of the fp32 oracle against the fp64 oracle on the same sample.  States: the
error against fp64 at the 99.9th percentile and at the maximum is at most C_RULE x the fp32 oracle's own error on the same entries, plus
the floors 1e-7 and 1e-6 (accumulate / assert_c_rule); the cached impulses of the warm-start slots enter as three more fields (box /
ground slots that hold the same corner, hand slots and joint-limit slots valid in all three), and the set of valid hand and limit
slots is exact.  An env that the two oracles alone decide differently (oracles_differ), or whose free step the fp64 oracle alone shows
to be decided by float32 roundoff (roundoff_decided), is left out, within the same cap.  A helper
that takes a tolerance has no default for it: the tests state them."""
import contextlib
import functools
import math
import os

import numpy as np

from dexrobot_isaac_amd.config import build_sim_config, default_cfg
from dexrobot_isaac_amd.hand_model import HandModel, rot_z
from tests import generic_model
from tests import tumbled_states as ts
from tests.tumbled_states import f32

N, SEED = 256, 11                  # the tumbled samples: four workgroups, every box class in each
C_RULE = 3.0                       # test_gpu_parity.py::test_hip_error_is_a_small_multiple_of_fp32_roundoff derives it
LEFT_OUT = 0.02
SYNC = ("q", "qd", "box_pos", "box_quat", "box_lin", "box_ang")
FIELDS = SYNC + ("cforce",)
BOX_FIELDS = ("box_pos", "box_quat", "box_lin", "box_ang")


# ------------------------------------------------------------------------------------------------- hand models without the folded structure
SWITCH = "DEXSIM_GENERAL_MODEL_PATH"


@contextlib.contextmanager
def general_path():
    """dexsim_create inside the block clears the model classification (tests/test_model_structure.py)."""
    old = os.environ.get(SWITCH)
    os.environ[SWITCH] = "1"
    try:
        yield
    finally:
        if old is None:
            del os.environ[SWITCH]
        else:
            os.environ[SWITCH] = old


def _tilt_axis(m, j):          # a flexion axis tilted by 1e-2 rad, renormalised
    a = np.array([0.0, -math.cos(1e-2), math.sin(1e-2)])
    m.jaxis[j] = a / np.linalg.norm(a)


def _break_poff4(m):
    m.jpoff[4] = (0.0, 2e-3, 0.0)


def _break_axis(m):
    _tilt_axis(m, 6 + 4 * 1 + 1)


def _break_qoff(m):
    j = 6 + 4 * 2 + 2
    m.jRoff[j] = m.jRoff[j] @ rot_z(1e-2)


def _break_com(m):
    m.com[6 + 4 * 3 + 2, 1] = 1e-3


def _break_all(m):
    _break_poff4(m), _break_axis(m), _break_qoff(m), _break_com(m)


def _mixed(m):                 # fingers 1 and 3 lack the structure, 2 and 4 (and the thumb) keep it
    m.com[6 + 4 * 1 + 3, 1] = 1e-3
    _tilt_axis(m, 6 + 4 * 3 + 2)


_ROT = (math.sin(0.05) / math.sqrt(2.0), math.sin(0.05) / math.sqrt(2.0), 0.0, math.cos(0.05))   # 0.1 rad about (1, 1, 0)
MODELS = {
    "poff4": (_break_poff4, None), "axis": (_break_axis, None), "qoff": (_break_qoff, None), "com": (_break_com, None),
    "hand_rot": (None, _ROT), "all": (_break_all, _ROT), "mixed": (_mixed, None),
    # none of the default model's zeros, ones and repeated numbers, by tenths of a radian and a centimetre (it turns the spawn frame itself)
    "generic": (generic_model.generic, None),
}


def _model_edit(name):
    """(edit, rot) of a name of MODELS, or of "generic:<property>": the generic model with that property of generic_model.RESTORE put
    back to the default model's value (the bite test of tests/test_generic_model.py)."""
    if name in MODELS:
        return MODELS[name]
    base, prop = name.split(":", 1)
    assert base == "generic"

    def edit(m):
        generic_model.generic(m)
        if generic_model.RESTORE[prop] is not None:
            generic_model.RESTORE[prop](m)
    return edit, None


# ------------------------------------------------------------------------------------------------- configuration
@functools.lru_cache(maxsize=None)
def setup(task, n, model=None, ground_friction=None, hand_friction=None, **over):
    """(sc, model, ms) of n envs, built once per process.  `over`: dotted keys into default_cfg(task), list indices included
    ("sim.gravity.0"); `model`: a name of MODELS or "generic:<property>" (_model_edit); ground_friction (hard-wired in config.py) and hand_friction (fixed by the MJCF-less
    model) are set on the built DexSimConfig / HandModel before to_struct()."""
    cfg = default_cfg(task)
    cfg["env"]["numEnvs"] = n
    for key, value in over.items():
        d, parts = cfg, key.split(".")
        for p in parts[:-1]:
            d = d[p]
        d[int(parts[-1]) if isinstance(d, list) else parts[-1]] = value
    hand = None
    if model is not None:
        edit, rot = _model_edit(model)
        if rot is not None:
            cfg["env"]["initialHandRot"] = list(rot)
        hand = HandModel(cfg["env"]["initialHandPos"], cfg["env"]["initialHandRot"])
        if edit is not None:
            edit(hand)
    sc, hand = build_sim_config(cfg, model=hand)
    if ground_friction is not None:
        sc.ground_friction = ground_friction
    if hand_friction is not None:
        hand.hand_friction = hand_friction
    return sc, hand, hand.to_struct()


# ------------------------------------------------------------------------------------------------- backends and state
def load(b, st):
    for k, v in st.items():
        b.set(k, v)


def hip(sc, ms, fused=True):
    from tests.hip_backend import HipBackend
    return HipBackend(sc, ms, fused=fused)


def backends(sc, ms, st=None, f64=False, fused=True, threads=0):
    """(fp32 oracle, HipBackend) -- with f64 = True (fp64 oracle, fp32 oracle, HipBackend) -- each loaded with the state `st`."""
    from oracle.oracle import Oracle
    out = ((Oracle(sc, ms, f64=True, threads=threads),) if f64 else ()) + (Oracle(sc, ms, threads=threads), hip(sc, ms, fused))
    for b in out:
        load(b, st or {})
    return out


def random_state(rng, model, n, near_box=True):
    """A spread of physically meaningful states: hand above / beside / pressing on the box."""
    q = rng.uniform(0.0, 0.5, (26, n))
    q[:3] = rng.uniform(-0.15, 0.15, (3, n))
    q[2] = rng.uniform(-0.42, -0.2, n) if near_box else rng.uniform(-0.2, 0.2, n)
    q[3:6] = rng.uniform(-0.3, 0.3, (3, n))
    q = np.clip(q, model.lo[:, None] + 1e-3, model.hi[:, None] - 1e-3)
    qd = rng.normal(0, 0.3, (26, n))
    tg = q + rng.normal(0, 0.05, (26, n))
    box_pos = np.stack([rng.uniform(-0.03, 0.03, n), rng.uniform(-0.03, 0.03, n), rng.uniform(0.0245, 0.03, n)])
    yaw = rng.uniform(-np.pi, np.pi, n)
    box_quat = np.stack([0 * yaw, 0 * yaw, np.sin(yaw / 2), np.cos(yaw / 2)])
    return dict(q=q, qd=qd, targets=tg, box_pos=box_pos, box_quat=box_quat,
                box_lin=rng.normal(0, 0.05, (3, n)), box_ang=rng.normal(0, 0.3, (3, n)))


def lowered_hand_state(rng, n, z, dz, rot):
    """The hand at rest, lowered to z + U(-dz, dz) over the upright box at rest at the origin: base rotations U(-rot, rot), finger
    joints U(0, 0.3), every target on its joint."""
    q = np.zeros((26, n))
    q[2] = z + rng.uniform(-dz, dz, n)
    q[3:6] = rng.uniform(-rot, rot, (3, n))
    q[6:] = rng.uniform(0, 0.3, (20, n))
    return dict(q=q, qd=0 * q, targets=q, box_pos=np.array([[0.0], [0.0], [0.0255]]) + 0 * q[:3],
                box_quat=np.array([[0.0], [0.0], [0.0], [1.0]]) + 0 * q[:4], box_lin=0 * q[:3], box_ang=0 * q[:3])


def tumbled_state(kind, n, seed=SEED, **cfg):
    """The first n envs of the N-env sample of tests/tumbled_states.py drawn for the BlindGrasping configuration setup(..., **cfg)."""
    sc, model, _ = setup("BlindGrasping", N, **cfg)
    return {k: v[:, :n].copy() for k, v in ts.sample(kind, N, seed, config=(sc, model)).items()}


def per_env_box(state, seed=23):
    """A copy of a sample's state with a box mass and a box friction of its own in every env: two more (1, n) rows, drawn in this
    order from default_rng(seed) -- box_mass U(0.05, 0.2) kg, box_mu U(0.5, 1.5), the ranges of the config-5 tests -- and rounded to
    float32 numbers, so that the fp64 oracle, the fp32 oracle and the kernels hold the same values.  load() sets them like any other
    key; teacher_ref puts only SYNC back between sub-steps, so they stay."""
    n = state["q"].shape[1]
    rng = np.random.default_rng(seed)
    box_mass = rng.uniform(0.05, 0.2, (1, n))
    box_mu = rng.uniform(0.5, 1.5, (1, n))
    return {**{k: v.copy() for k, v in state.items()}, "box_mass": f32(box_mass), "box_mu": f32(box_mu)}


class Oracle32:
    """The fp32 oracle in the kernels' place (the stand-ins of the CPU tests that show a comparison bites are its subclasses)."""

    def __init__(self, sc, ms):
        from oracle.oracle import Oracle
        self.o, self.subs, self.taken = Oracle(sc, ms), int(sc.substeps), 0

    def __getattr__(self, name):
        return getattr(self.o, name)

    def substep(self, last=True):
        self.o.substep(last=last)
        self.taken += 1

    def physics_step(self):
        for sub in range(self.subs):
            self.substep(last=sub == self.subs - 1)


# ------------------------------------------------------------------------------------------------- snapshots
def lists(b, n):
    return [b.contacts(e).copy() for e in range(n)]


def bg_cache(b):
    """Warm-start cache of the box / ground slots 80-83: impulses (12, n) and the corner each slot holds (4, n), -1 = not valid."""
    lam, tag, gen = b.warm_cache()
    tag = tag[80:84]
    return lam[240:252].copy(), np.where((tag >> 3) == gen[None, :], tag & 7, -1)


def snap(b, fields=FIELDS):
    """The fields, the list lengths and the warm-start cache by groups of slots: box / ground (bg_cache), hand contacts (slots 0-79:
    three impulses each) and joint-limit rows (slots 88 and above: one impulse each), with whether each slot's tag is valid for the
    env's generation."""
    s = {f: b.get(f) for f in fields}
    s["ncontact"] = b.get("ncontact")[0].astype(int)
    s["lam"], s["corner"] = bg_cache(b)
    lam, tag, gen = b.warm_cache()
    valid = (tag >> 3) == gen[None, :]
    s["hlam"], s["hvalid"] = lam[:240].copy(), valid[:80]
    s["llam"], s["lvalid"] = lam[264::3].copy(), valid[88:]
    return s


CACHE_GROUPS = (("wlam hand", "hlam", "hvalid", 3), ("wlam limit", "llam", "lvalid", 1))
SNAP_EXTRAS = ("ncontact", "lam", "corner", "hlam", "hvalid", "llam", "lvalid")          # what snap() adds to the fields


# ------------------------------------------------------------------------------------------------- references, computed once
def oracles_differ(s64, s32, ms):
    """(n,) the envs that the two oracles alone decide differently, by roundoff: another list length, another set of valid cache
    slots, or a joint that ends the sub-step clamped on a stop in one and free in the other (its qd then differs by the whole
    speed, not by roundoff).  Computed from the references only: such an env may be left out of a comparison, LEFT_OUT at the most."""
    lo = np.array(np.ctypeslib.as_array(ms.lo), dtype=np.float64)[:, None]      # the float32 limits every side clamps at
    hi = np.array(np.ctypeslib.as_array(ms.hi), dtype=np.float64)[:, None]
    stop = ((s64["q"] <= lo) != (s32["q"] <= lo)) | ((s64["q"] >= hi) != (s32["q"] >= hi))
    slots = (s64["hvalid"] != s32["hvalid"]).any(0) | (s64["lvalid"] != s32["lvalid"]).any(0)
    return (s64["ncontact"] != s32["ncontact"]) | slots | stop.any(0)


def left_by_the_references(recs):
    """(n,) the envs that oracles_differ names in any record; the cap is asserted here, before anything under test is read."""
    left = np.any([rec["left"] for rec in recs], axis=0)
    assert left.mean() <= LEFT_OUT, f"the oracles alone leave out {left.sum()} of {left.size} envs"
    return left


def teacher_ref(sc, ms, start):
    """Three teacher-forced sub-steps on the fp64 and the fp32 oracle (fresh instances): after each, q, qd and the box state of both
    are put to the fp64 oracle's values rounded to float32, so that every sub-step starts from one state.  Per sub-step: the
    float32 state it started from, both snapshots, the envs the oracles decide differently (oracles_differ) and (first sub-step)
    both contact lists."""
    from oracle.oracle import Oracle
    n = int(sc.num_envs)
    o64, o32 = Oracle(sc, ms, f64=True), Oracle(sc, ms)
    load(o64, start), load(o32, start)
    out = []
    for sub in range(3):
        o64.substep(last=True), o32.substep(last=True)
        rec = dict(start=start, s64=snap(o64), s32=snap(o32))
        rec["left"] = oracles_differ(rec["s64"], rec["s32"], ms)
        if sub == 0:
            rec["lists64"], rec["lists32"] = lists(o64, n), lists(o32, n)
            _, rec["wtag64"], rec["wgen64"] = o64.warm_cache()
        out.append(rec)
        start = {k: f32(o64.get(k)) for k in SYNC}
        load(o64, start), load(o32, start)
    return out


@functools.lru_cache(maxsize=None)
def tumbled_teacher_ref(kind, n, seed=SEED, **cfg):
    """teacher_ref of the tumbled sample `kind`, first n envs, at the configuration setup("BlindGrasping", n, **cfg)."""
    sc, _, ms = setup("BlindGrasping", n, **cfg)
    return teacher_ref(sc, ms, tumbled_state(kind, n, seed, **cfg))


@functools.lru_cache(maxsize=None)
def tumbled_free_ref(kind, n, steps, fields=FIELDS, seed=SEED, **cfg):
    """The tumbled sample free-running for `steps` physics steps (sim.substeps sub-steps each) on both oracles: snapshots after each."""
    sc, _, ms = setup("BlindGrasping", n, **cfg)
    return free_run_ref(sc, ms, tumbled_state(kind, n, seed, **cfg), steps, fields)


def free_run_ref(sc, ms, start, steps, fields=FIELDS):
    """`start` free-running for `steps` physics steps (sim.substeps sub-steps each) on both oracles: snapshots after each."""
    from oracle.oracle import Oracle
    o64, o32 = Oracle(sc, ms, f64=True), Oracle(sc, ms)
    load(o64, start), load(o32, start)
    out = []
    for _ in range(steps):
        o64.physics_step(), o32.physics_step()
        out.append(dict(s64=snap(o64, fields), s32=snap(o32, fields)))
    return out


def free_step_ref(sc, ms, start):
    """One free-running physics step (sim.substeps sub-steps) from `start` on both oracles: the snapshots after it and `left`, the
    envs that oracles_differ names after any of its sub-steps."""
    from oracle.oracle import Oracle
    o64, o32 = Oracle(sc, ms, f64=True), Oracle(sc, ms)
    load(o64, start), load(o32, start)
    left, subs = np.zeros(int(sc.num_envs), bool), int(sc.substeps)
    for sub in range(subs):
        o64.substep(last=sub == subs - 1), o32.substep(last=sub == subs - 1)
        s64, s32 = snap(o64), snap(o32)
        left |= oracles_differ(s64, s32, ms)
    return dict(start=start, s64=s64, s32=s32, left=left)


# ------------------------------------------------------------------------------------------------- comparisons: contact lists
def same_lists(a, b):
    return a.shape == b.shape and bool((a[:, 8] == b[:, 8]).all()) and bool((a[a[:, 8] != 2, 9] == b[a[:, 8] != 2, 9]).all())


def assert_same_entries(co, ch, atol):
    """The list `ch` under test against the oracle's `co`, entry by entry: type exact, capsule id of the hand entries exact (it is
    undefined for box / ground), point, normal, gap and friction within atol."""
    assert co.shape == ch.shape
    assert (co[:, 8] == ch[:, 8]).all()
    hand = co[:, 8] != 2
    assert (co[hand, 9] == ch[hand, 9]).all()
    np.testing.assert_allclose(ch[:, :8], co[:, :8], atol=atol)


def dist(row, sc, ms):
    """gap + rest_offset + capsule radius of a hand / box entry: the distance of the axis point from the box."""
    return row[6] + float(sc.rest_offset) + float(ms.cap_r[int(row[9])])


def normal_scale(lists64, lists32, envs, sc, ms):
    """E: the largest err_n dist of the fp32 oracle's hand / box normals against the fp64 oracle's."""
    E = 0.0
    for e in envs:
        for r64, r32 in zip(lists64[e], lists32[e]):
            if r64[8] == 1:
                E = max(E, np.abs(r32[3:6] - r64[3:6]).max() * dist(r64, sc, ms))
    return E


def agree(same, *counts, exact=True):
    for a in counts[1:]:
        same = same & (counts[0] == a)
    assert not exact or 1.0 - same.mean() <= LEFT_OUT, f"{(~same).sum()} of {same.size} envs left out"
    return same


def check_manifold(b, rec, sc, ms, keep=None):
    """The backend under test `b` has taken the first teacher-forced sub-step of a hand-on-box sample: its list of every env (of the
    envs `keep`) against the fp64 oracle's."""
    n = len(rec["lists64"])
    got = lists(b, n)
    same = agree(np.ones(n, bool) if keep is None else keep, rec["s64"]["ncontact"], rec["s32"]["ncontact"], np.array([len(c) for c in got]))
    envs = np.nonzero(same)[0]
    _, corner = bg_cache(b)
    assert (corner[:, same] == rec["s64"]["corner"][:, same]).all(), "a box / ground slot holds another corner"
    E = normal_scale(rec["lists64"], rec["lists32"], envs, sc, ms)
    worst, worst_pg, entries = 0.0, 0.0, 0
    for e in envs:
        co, ch = rec["lists64"][e], got[e]
        assert same_lists(co, ch), e                                             # type, and capsule of the hand entries
        if not len(co):
            continue
        worst_pg = max(worst_pg, np.abs(ch[:, [0, 1, 2, 6]] - co[:, [0, 1, 2, 6]]).max())
        np.testing.assert_allclose(ch[:, [0, 1, 2, 6, 7]], co[:, [0, 1, 2, 6, 7]], rtol=0, atol=2e-6)
        for ro, rh in zip(co, ch):
            err = np.abs(rh[3:6] - ro[3:6]).max()
            if ro[8] == 1:
                d = dist(ro, sc, ms)
                worst = max(worst, err * d)
                assert err <= C_RULE * E / d + 1e-7, (e, int(ro[9]), err, d, E)
            else:
                assert err <= 1e-7, (e, err)                                     # the ground's normal
        entries += len(co)
    print(f"\n{entries} entries in {len(envs)} envs; E = {E:.3e} m, worst err_n dist under test {worst:.3e} m, points / gaps {worst_pg:.2e}")
    assert entries > 3 * n


def check_pressed_lists(make, rec, label):
    """The backend that make() returns takes the first teacher-forced sub-step of a sample whose fingers are pressed into the box
    (check_manifold's E / dist bound takes an axis point outside it): the list of every env entry by entry, joint-limit rows
    included -- type and capsule / joint level exact, points, gaps and friction to 2e-6, box / ground slot corners exact; the normals
    as one more field of the c rule.  Returns the kept envs and the lists under test."""
    n = len(rec["lists64"])
    keep = ~left_by_the_references([rec])
    b = make()
    load(b, rec["start"])
    b.substep(last=True)
    got = lists(b, n)
    keep = agree(keep, rec["s64"]["ncontact"], np.array([len(c) for c in got]))
    assert (bg_cache(b)[1][:, keep] == rec["s64"]["corner"][:, keep]).all(), "a box / ground slot holds another corner"
    for e in np.nonzero(keep)[0]:
        assert same_lists(rec["lists64"][e], got[e]), e
    l64, l32, lh = (np.concatenate([l[e] for e in np.nonzero(keep)[0]]) for l in (rec["lists64"], rec["lists32"], got))
    worst = np.abs(lh[:, [0, 1, 2, 6, 7]] - l64[:, [0, 1, 2, 6, 7]]).max()
    print(f"\n{label}: {len(l64)} entries in {keep.sum()} envs, points / gaps / friction within {worst:.2e}")
    np.testing.assert_allclose(lh[:, [0, 1, 2, 6, 7]], l64[:, [0, 1, 2, 6, 7]], rtol=0, atol=2e-6)
    report = {}
    accumulate(report, "normals", l64[:, 3:6], l32[:, 3:6], lh[:, 3:6], np.ones((len(l64), 3), bool))
    assert_c_rule(report, f"lists, {label}, n = {n}")
    assert len(l64) > 10 * n
    return keep, got


def expected_friction(c, e, start, sc, ms):
    """The friction column of env e's list `c` as the specification has it, from the state's own box_mu row (the configuration's
    box_friction without one): the mean of the two surfaces' coefficients -- hand / ground (type 0), hand / box (1), box / ground (2)."""
    bmu = float(start["box_mu"][0, e]) if "box_mu" in start else float(sc.box_friction)
    hand, ground = float(ms.hand_friction), float(sc.ground_friction)
    return np.select([c[:, 8] == 0, c[:, 8] == 1, c[:, 8] == 2], [0.5 * (hand + ground), 0.5 * (hand + bmu), 0.5 * (bmu + ground)], np.nan)


def check_friction_column(got, rec, keep, atol, types=(1, 2)):
    """The friction of every hand / box (type 1) and box / ground (type 2) entry of the lists `got` against the fp64 oracle's, per
    entry, over the envs `keep` whose lists agree entry for entry: within atol; each of `types` must occur."""
    for typ, name in ((1, "hand / box"), (2, "box / ground")):
        if typ not in types:
            continue
        err = np.concatenate([np.abs(got[e][:, 7] - rec["lists64"][e][:, 7])[rec["lists64"][e][:, 8] == typ] for e in np.nonzero(keep)[0]])
        assert err.size > 0, name
        print(f"friction of {err.size} {name} entries within {err.max():.2e}")
        assert err.max() <= atol, (name, float(err.max()))


# ------------------------------------------------------------------------------------------------- comparisons: states by the c rule
def accumulate(report, name, ref, a32, ah, mask):
    e32, eh = np.abs(a32 - ref)[mask].ravel(), np.abs(ah - ref)[mask].ravel()
    if not e32.size:
        return
    r = report.setdefault(name, [0.0, 0.0, 0.0, 0.0])
    r[0], r[1] = max(r[0], np.percentile(e32, 99.9)), max(r[1], np.percentile(eh, 99.9))
    r[2], r[3] = max(r[2], e32.max()), max(r[3], eh.max())


def accumulate_snap(report, s64, s32, sh, same, fields):
    for f in fields:
        accumulate(report, f, s64[f], s32[f], sh[f], np.broadcast_to(same, s64[f].shape))
    # cached impulses of the box / ground slots that hold the same corner in all three
    ok = (s64["corner"] >= 0) & (s64["corner"] == s32["corner"]) & (s64["corner"] == sh["corner"]) & same
    accumulate(report, "wlam 80-83", s64["lam"], s32["lam"], sh["lam"], np.repeat(ok, 3, axis=0))
    # ... and of the hand slots and the joint-limit slots that are valid in all three
    for name, lam, valid, rows in CACHE_GROUPS:
        ok = s64[valid] & s32[valid] & sh[valid] & same
        accumulate(report, name, s64[lam], s32[lam], sh[lam], np.repeat(ok, rows, axis=0))


def assert_same_slots(sh, s64, same):
    """The snapshot under test holds valid hand and joint-limit cache slots exactly where the fp64 oracle's does, over the envs `same`."""
    for _, _, valid, _ in CACHE_GROUPS:
        bad = (sh[valid] != s64[valid]).any(0) & same
        assert not bad.any(), f"{valid}: the set of valid cache slots differs in {bad.sum()} envs, first {np.nonzero(bad)[0][:8]}"


def c_rule_factor(report):
    """By what factor the report misses (> 1) or meets (<= 1) the rule: the largest error over its bound."""
    return max(max(r[1] / (C_RULE * r[0] + 1e-7), r[3] / (C_RULE * r[2] + 1e-6)) for r in report.values())


def assert_c_rule(report, label):
    print(f"\n{label}\nfield: p99.9 |f32-f64|, p99.9 |under test-f64|, max |f32-f64|, max |under test-f64|, ratios")
    for f, r in report.items():
        print(f"  {f:10s} {r[0]:.3e} {r[1]:.3e} {r[2]:.3e} {r[3]:.3e}   {r[1] / max(r[0], 1e-30):.2f} {r[3] / max(r[2], 1e-30):.2f}")
    for f, r in report.items():
        assert r[1] <= C_RULE * r[0] + 1e-7, (f, r)
        assert r[3] <= C_RULE * r[2] + 1e-6, (f, r)


def teacher_forced_report(make, recs, kind, exact=True):
    """The backend that make() returns through the teacher-forced sub-steps of the references `recs` (teacher_ref): contact counts
    over the envs that agree, slot corners and the sets of valid hand and limit slots exact; the report for the c rule.
    exact = False skips the exact assertions on the output under test, for the margins of the stand-ins."""
    same, report = ~left_by_the_references(recs), {}
    b = make()
    for rec in recs:
        load(b, rec["start"])
        b.substep(last=True)
        sh = snap(b)
        if kind == "box_alone":
            assert sh["ncontact"].max() <= 4 and rec["s64"]["ncontact"].max() <= 4       # the early box solve really ran
        same = agree(same, rec["s64"]["ncontact"], rec["s32"]["ncontact"], sh["ncontact"], exact=exact)   # (an env left out stays out: its cache differs)
        assert not exact or (sh["corner"][:, same] == rec["s64"]["corner"][:, same]).all(), "a box / ground slot holds another corner"
        if exact:
            assert_same_slots(sh, rec["s64"], same)
        accumulate_snap(report, rec["s64"], rec["s32"], sh, same, FIELDS)
    return report


def check_teacher_forced(make, recs, kind, label=""):
    """teacher_forced_report, then states and cached impulses by the c rule."""
    report = teacher_forced_report(make, recs, kind)
    assert_c_rule(report, f"teacher-forced, {label}{kind}, n = {recs[0]['s64']['ncontact'].size}")
    assert "wlam 80-83" in report
    return report


def check_free_step(sh, ref, where=""):
    """The snapshot `sh` under test after a free-running physics step against both oracles' (a record of tumbled_free_ref): contact
    counts and slot corners exact in every env."""
    for s in (ref["s64"], ref["s32"]):
        assert (sh["ncontact"] == s["ncontact"]).all(), f"contact count differs in {(sh['ncontact'] != s['ncontact']).sum()} envs{where}"
        assert (sh["corner"] == s["corner"]).all(), f"slots 80-83 differ in {(sh['corner'] != s['corner']).any(0).sum()} envs{where}"


def roundoff_decided(sc, ms, ref, draws=8):
    """(n,) the envs of a free_step_ref record in which float32 roundoff decides the step's result, by the two oracles alone.  The c
    rule takes the fp32 oracle's error on an entry for what float32 roundoff does to it.  Here the fp64 oracle repeats the physics step
    `draws` times from the start with every number of SYNC moved by a relative U(-2^-24, 2^-24), half a float32 ulp; an env is named
    when a state field of its then spreads, at the maximum over the draws, beyond the rule's own bound for that field, C_RULE x the
    fp32 oracle's largest error + 1e-6: there one realisation of roundoff (the fp32 oracle's) says nothing about another (a branch of
    the solver -- a cone, a clamp, an opening contact -- is taken or not by the last bit), and no implementation in float32 can be
    held to it.  Such an env may be left out of a comparison like one of oracles_differ, within the same cap."""
    from oracle.oracle import Oracle
    named = np.zeros(int(sc.num_envs), bool)
    spread = {f: np.zeros(int(sc.num_envs)) for f in SYNC}
    for draw in range(draws):
        rng = np.random.default_rng(draw)
        o = Oracle(sc, ms, f64=True)
        load(o, {k: v * (1.0 + 2.0 ** -24 * rng.uniform(-1.0, 1.0, v.shape)) if k in SYNC else v for k, v in ref["start"].items()})
        o.physics_step()
        for f in SYNC:
            spread[f] = np.maximum(spread[f], np.abs(o.get(f) - ref["s64"][f]).max(0))
    for f in SYNC:
        named |= spread[f] > C_RULE * np.abs(ref["s32"][f] - ref["s64"][f]).max() + 1e-6
    return named


def free_step_report(make, ref, exact=True):
    """One free-running physics step of the backend that make() returns from the start of `ref` (free_step_ref) against both
    oracles: contact counts, slot corners and valid-slot sets where the oracles agree; the report.  exact = False skips the exact
    assertions on the output under test, for the stand-ins' margins."""
    assert ref["left"].mean() <= LEFT_OUT, f"the oracles alone leave out {ref['left'].sum()} of {ref['left'].size} envs"
    b = make()
    load(b, ref["start"])
    b.physics_step()
    sh = snap(b)
    same = agree(~ref["left"], ref["s64"]["ncontact"], ref["s32"]["ncontact"], sh["ncontact"], exact=exact)
    if exact:
        assert (sh["corner"][:, same] == ref["s64"]["corner"][:, same]).all(), "a box / ground slot holds another corner"
        assert_same_slots(sh, ref["s64"], same)
    report = {}
    accumulate_snap(report, ref["s64"], ref["s32"], sh, same, FIELDS)
    return report


# ------------------------------------------------------------------------------------------------- comparisons: whole control steps
def random_actions(rng, n, scale=1.0):
    return (scale * (2 * rng.random((n, 18)) - 1)).astype(np.float32)


def control_steps(o, hb, rng, steps, reset_atol, obs_bar, rew_atol, rew_rtol, q_atol):
    """reset and `steps` random-action control steps with in-step resets of the backend `hb` against the fp32 oracle `o`: done flags
    and the reset count of every step exact, two physics steps exactly where an env was reset, rewards and the final q within
    their tolerances, the worst observation error of the run below obs_bar, and more resets than envs."""
    n = o.n
    np.testing.assert_allclose(hb.reset(), o.reset(), atol=reset_atol)
    worst = 0.0
    for t in range(steps):
        a = random_actions(rng, n)
        oo, ro, do = o.step(a)
        oh, rh, dh = hb.step(a)
        assert (do == dh.astype(bool)).all(), t
        assert hb.stats()[16] == o.stats()[16] and hb.stats()[17] == (2 if do.any() else 1)
        worst = max(worst, float(np.abs(oh - oo).max()))
        np.testing.assert_allclose(rh, ro, atol=rew_atol, rtol=rew_rtol)
    assert worst < obs_bar, worst
    assert o.get("reset_count").sum() > n
    np.testing.assert_allclose(hb.get("q"), o.get("q"), atol=q_atol)


def free_running(o, hb, rng, steps, reset_atol, median, p99, mismatches, resets, twin=None, label=None):
    """reset and `steps` free-running random-action control steps of `hb` against the fp32 oracle `o`.  fp32 roundoff grows through
    contacts, so the bars are statistical for trajectories (median and 99th percentile of the per-env observation error) and a count
    for the integer bookkeeping (done mismatches in all, reset count per step).  `twin`: a second backend that must give hb's values
    with `==` in every step."""
    n = o.n
    obs_o, obs_h = o.reset(), hb.reset()
    np.testing.assert_allclose(obs_h, obs_o, atol=reset_atol)
    assert twin is None or (obs_h == twin.reset()).all()
    errs, mism = [], 0
    for t in range(steps):
        a = random_actions(rng, n)
        oo, ro, do = o.step(a)
        oh, rh, dh = hb.step(a)
        if twin is not None:
            og, rg, dg = twin.step(a)
            assert (oh == og).all() and (rh == rg).all() and (dh == dg).all(), f"step {t}: the switch changes values"
        errs.append(np.abs(oh - oo).max(axis=1))
        mism += int((do != dh.astype(bool)).sum())
        assert abs(hb.stats()[16] - o.stats()[16]) <= resets     # resets this step
    errs = np.stack(errs)
    if label is not None:
        print(f"{label}: median {np.median(errs):.3g}  p99 {np.percentile(errs, 99):.3g}  done mismatches {mism}")
    assert np.median(errs) < median
    assert np.percentile(errs, 99) < p99
    assert mism <= mismatches
    assert o.get("reset_count").sum() > n                    # resets (timeouts) really happened
