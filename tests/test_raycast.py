"""Range sensors on the device (dexsim_raycast, env.create_ray_sensor / read_ray_sensor) against tests/raycast_ref.py, a numpy
statement of the rule include/dexsim_ray.h specifies, run in float64 and, for the roundoff figures, in float32.

The main set (raycast_ref.make_poses / make_rays): 70 poses by the recipe of the camera tests -- hand lowered to ~0.10 m above the
ground, finger joints over their ranges, base rotations +-0.25 rad, box within +-3 cm of the capsule centroid with a random
orientation -- and 87 rays: four from every fingertip site and three from every pad site on the distal joint frames, two 4 x 4 fans
from the palm frame, eight rays that start above a capsule of their own parent frame and point back through it, twelve world rays
aimed at the mean box position.  min_range 0.03 m, max_range 1 m.  Everything is rounded to float32 before either side sees it.

Rules of every comparison (raycast_ref.compare):
  * rays the reference marks unstable (id changes under +-0.2 mm inflation, box edges, t within 1e-3 relative of the window's ends,
    ground hits with |d_z| < 1e-3) are left out; at most 8 % of the rays of any env and 3 % of all may be unstable -- asserted on
    the reference alone before any GPU output is read;
  * segment ids: exact;
  * t, hit point, normal components: ten times the error the SAME reference makes in float32 on the same inputs, computed here on
    the CPU and printed, never taken from the code under test (the rule and the factor of tests/test_render.py, whose docstring
    gives the reason for the ten) -- absolute on hand and box hits, relative to t on the ground.
Every GPU test uses N = 70: two workgroups, six live lanes in the second.  Every device output sits between two guard rows that must
come back untouched.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from dexrobot_isaac_amd import _abi
from tests import raycast_ref as rc
from tests import render_ref as rr
from tests.query_rig import bits, load_lib, pose_core, purity_frame, setup, stub_core

N = rc.ROWS
NJ, NCAP = _abi.NJ, _abi.NCAP
GROUND, BOX, CAP0, NONE = _abi.SEG_GROUND, _abi.SEG_BOX, _abi.SEG_CAPSULE0, _abi.SEG_NONE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = int(re.search(r"#define RC_CHUNK (\d+)", open(os.path.join(ROOT, "dexrobot_isaac_amd", "csrc", "dexsim_raycast.hip.inc")).read()).group(1))
MAX_UNSTABLE_ENV, MAX_UNSTABLE_ALL = 0.08, 0.03


# ------------------------------------------------------------------------------------------------- CPU
@pytest.fixture(scope="module")
def lib():
    return load_lib()


def test_abi_exports_and_argument_errors(lib):
    """include/dexsim_ray.h, the part of the header the entry point is declared in, against _abi.RAY_PROTOTYPES and the built library, as
    tests/test_forward_kinematics.py holds dexsim_fk.h: the same names, the same number of parameters; then the argument errors."""
    inc = os.path.join(ROOT, "include")
    hdr, main_hdr = open(os.path.join(inc, "dexsim_ray.h")).read(), open(os.path.join(inc, "dexsim.h")).read()
    assert main_hdr.index("dexsim_render(") < main_hdr.index('#include "dexsim_ray.h"') < main_hdr.index("dexsim_body_jacobian(")   # behind the camera's
    assert "dexsim_raycast" not in open(os.path.join(inc, "dexsim_fk.h")).read()
    assert set(re.findall(r"\b(dexsim_[a-z_]+)\s*\(", hdr)) == set(_abi.RAY_PROTOTYPES) == {"dexsim_raycast"}
    declared = re.findall(r"\b(dexsim_[a-z_]+)\s*\(([^()]*)\)\s*;", hdr)
    assert [name for name, _ in declared] == list(_abi.RAY_PROTOTYPES)
    for name, params in declared:
        assert len(params.split(",")) == len(_abi.RAY_PROTOTYPES[name]), name
    assert not set(_abi.RAY_PROTOTYPES) & (set(_abi.PROTOTYPES) | set(_abi.FK_PROTOTYPES))
    assert hasattr(lib, "dexsim_raycast"), "libdexsim.so does not export dexsim_raycast"
    assert lib.dexsim_raycast.argtypes == _abi.RAY_PROTOTYPES["dexsim_raycast"]
    assert (_abi.RAY_MAX, _abi.RAY_SKIP_PARENT) == (4096, 1)
    assert re.search(r"#define DEXSIM_RAY_MAX\s+4096\b", hdr) and re.search(r"#define DEXSIM_RAY_SKIP_PARENT\s+1\b", hdr)

    buf = (C.c_float * 64)()
    base = C.addressof(buf)
    base += (-base) % 16
    p, odd = C.c_void_p(base), C.c_void_p(base + 4)                            # never written: every call below fails before a launch
    two = (C.c_int * 2)(0, 5)

    def call(h=None, k=1, size=0.0, rays=p, parent=two, nrays=2, lo=0.0, hi=1.0, flags=0, dist=p, hits=p):
        rcode = lib.dexsim_raycast(h, None, k, None, None, size, rays, parent, nrays, lo, hi, flags, dist, hits, None)
        return rcode, lib.dexsim_last_error()

    inf, nan = float("inf"), float("nan")
    cases = [
        (dict(), b"null handle"),
        (dict(k=0), b"k must be positive"), (dict(k=-3), b"k must be positive"),
        (dict(nrays=0), b"nrays"), (dict(nrays=_abi.RAY_MAX + 1), b"nrays"), (dict(nrays=-1), b"nrays"),
        (dict(rays=None), b"rays and parent"), (dict(parent=None), b"rays and parent"),
        (dict(parent=(C.c_int * 2)(-2, 0)), b"outside"), (dict(parent=(C.c_int * 2)(0, NJ)), b"outside"),
        (dict(parent=(C.c_int * 2)(5, 4)), b"non-decreasing"), (dict(parent=(C.c_int * 2)(0, -1)), b"non-decreasing"),
        (dict(lo=nan), b"ranges"), (dict(hi=inf), b"ranges"), (dict(lo=-0.1), b"ranges"), (dict(lo=0.5, hi=0.5), b"ranges"),
        (dict(lo=0.6, hi=0.5), b"ranges"), (dict(hi=nan), b"ranges"),
        (dict(flags=2), b"unknown flag"), (dict(flags=-1), b"unknown flag"),
        (dict(dist=None, hits=None), b"at least one"), (dict(dist=odd), b"16-byte aligned"), (dict(hits=odd), b"16-byte aligned"),
        (dict(dist=None, hits=odd), b"16-byte aligned"),
        (dict(size=nan), b"box_size"), (dict(size=inf), b"box_size"),
    ]
    for kw, text in cases:
        rcode, msg = call(**kw)
        assert rcode == 1 and text in msg, (kw, rcode, msg)                    # DEXSIM_ERR_ARG with its text
    assert not any(buf)


def test_reference_primitives():
    """ray_capsules / ray_boxes are render_ref's ray_capsule / ray_box with an origin per ray: equal on shared origins."""
    rng = np.random.default_rng(3)
    for _ in range(40):
        a, b = rng.uniform(-0.1, 0.1, 3), rng.uniform(-0.1, 0.1, 3)
        r = rng.uniform(0.005, 0.02)
        ro = rng.uniform(-0.2, 0.2, 3)
        rd = rr._unit(np.concatenate([(0.5 * (a + b) - ro)[None] + rng.normal(0, 0.01, (30, 3)), rng.normal(size=(10, 3))]))
        t0, n0 = rr.ray_capsule(ro, rd, a, b, r)
        t1, n1 = rc.ray_capsules(np.tile(ro, (40, 1)), rd, a, b, r)
        hit = np.isfinite(t0)
        assert (hit == np.isfinite(t1)).all() and hit.sum() >= 5
        assert np.abs(t0[hit] - t1[hit]).max() <= 1e-13 and np.abs(n0[hit] - n1[hit]).max() <= 1e-11
        c, R = rng.uniform(-0.1, 0.1, 3), rr.quat_to_mat(rng.normal(size=4))
        rd = rr._unit(np.concatenate([(c - ro)[None] + rng.normal(0, 0.02, (30, 3)), rng.normal(size=(10, 3))]))
        t0, n0, p0 = rr.ray_box(ro, rd, c, R, 0.03)
        t1, n1, p1 = rc.ray_boxes(np.tile(ro, (40, 1)), rd, c, R, 0.03)
        hit = np.isfinite(t0)
        assert (hit == np.isfinite(t1)).all() and hit.sum() >= 5 and np.abs(t0[hit] - t1[hit]).max() <= 1e-13
        assert np.abs(n0[hit] - n1[hit]).max() <= 1e-13 and np.abs(p0[hit] - p1[hit]).max() <= 1e-13


class _OneCapsule:
    """raycast_ref.cast over a single free-standing capsule (all 18 coincide) that rides on joint 5; every frame is the identity."""
    cap_r = np.full(NCAP, 0.01)
    cap_parent = np.full(NCAP, 5)

    def __init__(self, a, b):
        self.a, self.b = np.tile(a, (NCAP, 1)).astype(float), np.tile(b, (NCAP, 1)).astype(float)

    def fk(self, q, dtype=np.float64):
        return np.zeros((NJ, 3), dtype=dtype), np.tile(np.eye(3, dtype=dtype), (NJ, 1, 1))

    def capsules(self, q, dtype=np.float64):
        return self.a.astype(dtype), self.b.astype(dtype), None


def test_reference_closed_forms():
    q = np.zeros(NJ)
    g = _OneCapsule(np.array([0.5, 0.0, 1.0]), np.array([0.8, 0.0, 1.0]))
    one = lambda o, d, p=-1, **kw: {k: v[0] for k, v in rc.cast(g, q, kw.pop("box", None), np.array([[*o, *d]], dtype=float), [p], **kw).items()}
    # down the capsule's axis: the near end sphere, normal back along the ray; the direction is normalised
    r = one([0.0, 0.0, 1.0], [3.0, 0.0, 0.0], max_range=2.0)
    assert r["seg"] == CAP0 and abs(r["t"] - 0.49) < 1e-12 and np.abs(r["point"] - [0.49, 0, 1]).max() < 1e-12 and np.abs(r["normal"] - [-1, 0, 0]).max() < 1e-12
    # from the side onto the cylinder
    r = one([0.65, -0.4, 1.0], [0.0, 1.0, 0.0])
    assert r["seg"] == CAP0 and abs(r["t"] - 0.39) < 1e-12 and np.abs(r["normal"] - [0, -1, 0]).max() < 1e-12
    # starting inside the capsule: it is not seen, the ray goes on to the ground
    r = one([0.65, 0.0, 1.0], [0.0, 0.0, -1.0], max_range=2.0)
    assert r["seg"] == GROUND and abs(r["t"] - 1.0) < 1e-12 and np.abs(r["normal"] - [0, 0, 1]).max() < 1e-12
    # the range window: a hit before min_range does not count and does not stop the ray; one behind max_range is none
    assert one([0.65, -0.4, 1.0], [0.0, 1.0, 0.0], min_range=0.395)["seg"] == NONE
    assert one([0.65, 0.0, 1.5], [0.0, 0.0, -1.0], min_range=0.495, max_range=2.0)["seg"] == GROUND
    r = one([0.65, 0.0, 1.5], [0.0, 0.0, -1.0], max_range=0.4)
    assert r["seg"] == NONE and np.isposinf(r["t"]) and not r["point"].any() and not r["normal"].any()
    # the skip flag: a ray on the capsule's own frame passes through it, a world ray or one on another frame does not
    assert one([0.65, 0.0, 1.5], [0.0, 0.0, -1.0], 5, max_range=2.0, skip_parent=True)["seg"] == GROUND
    assert one([0.65, 0.0, 1.5], [0.0, 0.0, -1.0], 5, max_range=2.0)["seg"] == CAP0
    assert one([0.65, 0.0, 1.5], [0.0, 0.0, -1.0], -1, max_range=2.0, skip_parent=True)["seg"] == CAP0
    assert one([0.65, 0.0, 1.5], [0.0, 0.0, -1.0], 4, max_range=2.0, skip_parent=True)["seg"] == CAP0
    # onto a box face, and onto the ground at a known angle, from below as well
    box = (np.array([1.0, 0.0, 2.0]), np.array([0.0, 0.0, 0.0, 1.0]), 0.2)
    r = one([0.0, 0.0, 2.0], [1.0, 0.0, 0.0], box=box, max_range=2.0)
    assert r["seg"] == BOX and abs(r["t"] - 0.9) < 1e-12 and np.abs(r["normal"] - [-1, 0, 0]).max() < 1e-12
    assert one([1.0, 0.0, 2.0], [1.0, 0.0, 0.0], box=box, max_range=2.0)["seg"] == NONE          # from inside the cube
    pitch, z0 = np.radians(35.0), 0.7
    r = one([0.0, 5.0, z0], [np.cos(pitch), 0.0, -np.sin(pitch)], max_range=2.0)
    assert r["seg"] == GROUND and abs(r["t"] - z0 / np.sin(pitch)) < 1e-12 and abs(r["point"][2]) < 1e-15
    r = one([0.0, 5.0, -z0], [np.cos(pitch), 0.0, np.sin(pitch)], max_range=2.0)
    assert r["seg"] == GROUND and abs(r["t"] - z0 / np.sin(pitch)) < 1e-12 and np.abs(r["normal"] - [0, 0, 1]).max() == 0
    assert one([0.0, 5.0, z0], [0.0, 0.0, 0.0])["seg"] == NONE                                    # a zero direction never hits


# ------------------------------------------------------------------------------------------------- the reference on the main set
def _main_set(model):
    sc, ms = setup(N, model=model)
    geom = rr.HandGeometry(ms)
    q, box = rc.make_poses(geom)
    rays, parent = rc.make_rays(ms, box[:, :3].mean(0))
    world = rays[parent < 0]
    assert (np.abs(world[:, 5]) / np.linalg.norm(world[:, 3:], axis=1) > 1e-2).all()              # no world ray near the horizon
    refs = {skip: rc.reference_set(geom, q, box, rays, parent, skip_parent=skip) for skip in (False, True)}
    for skip, ref in refs.items():                                             # the conditions, on the reference alone
        u = ref["unstable"]
        print(f"skip_parent={skip}: unstable {u.mean(1).max():.3f} in the worst env, {u.mean():.3f} overall")
        assert u.mean(1).max() <= MAX_UNSTABLE_ENV and u.mean() <= MAX_UNSTABLE_ALL
    return dict(sc=sc, ms=ms, geom=geom, q=q, box=box, rays=rays, parent=parent, refs=refs,
                tols={skip: rc.tolerances(ref) for skip, ref in refs.items()})


@pytest.fixture(scope="module")
def main():
    return _main_set(None)


@pytest.fixture(scope="module")
def main_generic():
    return _main_set("generic")


def _roundoff_and_shares(S):
    seg = S["refs"][False]["seg"]
    share = {n: float(m.mean()) for n, m in (("ground", seg == GROUND), ("box", seg == BOX), ("capsule", seg >= CAP0), ("none", seg == NONE))}
    changed = int((S["refs"][False]["seg"] != S["refs"][True]["seg"]).sum())
    print("hit shares:", {k: f"{v:.3f}" for k, v in share.items()}, f"; {changed} rays change their answer with skip_parent")
    assert set((seg[seg >= CAP0] - CAP0).tolist()) == set(range(NCAP))                             # every capsule is hit in some env
    assert all(share[k] >= 0.05 for k in ("ground", "box", "capsule")) and changed >= 20
    for skip, tol in S["tols"].items():
        print(f"skip_parent={skip}: reference float32 against float64:", {k: f"{v:.3g}" for k, v in tol["err"].items()},
              f"; {tol['mismatch32']} id mismatches on stable rays")
        assert tol["mismatch32"] == 0
        # roundoff of fp32 numbers of metre size, not a flipped branch: far below the 0.2 mm stability margin
        assert 0 < tol["err"]["t_abs"] < 2e-5 and 0 < tol["err"]["t_rel"] < 2e-5 and 0 < tol["err"]["p_abs"] < 2e-5 and tol["err"]["n"] < 2e-3


def test_reference_roundoff_and_shares(main):
    _roundoff_and_shares(main)


def test_reference_roundoff_and_shares_generic_model(main_generic):
    _roundoff_and_shares(main_generic)


def _body_rays(hand):
    """Two rays from every pad and tip body, in the body's frame: (body index, origin, direction)."""
    rows = []
    for f in range(_abi.NFINGER):
        for name, dirs in ((f"r_f_link{f + 1}_pad", ([0.0, 0.0, 1.0], [0.3, 0.1, 1.0])), (f"r_f_link{f + 1}_tip", ([1.0, 0.0, 0.0], [1.0, 0.2, -0.3]))):
            rows += [(hand.body_names.index(name), [0.0, 0.0, 0.001], d) for d in dirs]
    return rows


def test_reference_discrimination(main):
    """The reference with one deliberate mistake misses the bound of the quantity it spoils: the ids (exact: any mismatch on a stable
    ray is a miss) or, on the rays whose id survives, t / point / normal by the printed factor of their bound."""
    S = main
    geom, q, box, rays, parent = S["geom"], S["q"], S["box"], S["rays"], S["parent"]
    boxes = [(box[e, :3], box[e, 3:], rc.BOX_SIZE) for e in range(N)]

    def miss(ref, tol, variant, rays=rays, parent=parent, skip=False):
        v = [rc.cast(geom, q[e], boxes[e], rays, parent, rc.MIN_RANGE, rc.MAX_RANGE, skip, variant=variant) for e in range(N)]
        seg, t = np.stack([x["seg"] for x in v]), np.stack([x["t"] for x in v])
        p, n = np.stack([x["point"] for x in v]), np.stack([x["normal"] for x in v])
        st = ~ref["unstable"]
        ids = int((seg != ref["seg"])[st].sum())
        same = st & (seg == ref["seg"]) & (seg != NONE)
        gnd = same & (seg == GROUND)
        obj = same & ~gnd
        t64 = np.where(same, ref["t"], 1.0)
        dt, dp = np.abs(np.where(same, t, 1.0) - t64), np.abs(p - ref["point"]).max(-1)
        f = {"t": max((dt[obj] / tol["t_abs"]).max(initial=0), ((dt / t64)[gnd] / tol["t_rel"]).max(initial=0)),
             "point": max((dp[obj] / tol["p_abs"]).max(initial=0), ((dp / t64)[gnd] / tol["p_rel"]).max(initial=0)),
             "normal": (np.abs(n - ref["normal"]).max(-1)[same] / tol["n"]).max(initial=0)}
        return ids, {k: float(x) for k, x in f.items()}

    found = {}
    found["dir_not_rotated"] = miss(S["refs"][False], S["tols"][False], "dir_not_rotated")
    found["min_range_ignored"] = miss(S["refs"][False], S["tols"][False], "min_range_ignored")
    found["exit_hit"] = miss(S["refs"][False], S["tols"][False], "exit_hit")
    found["skip_ignored"] = miss(S["refs"][True], S["tols"][True], "skip_ignored", skip=True)
    # body folding: sensors on the pad and tip bodies, folded with and without the body's offset
    hand = setup_hand()
    rows = _body_rays(hand)
    fold = lambda variant: [rc.fold_body(hand, b, o, d, variant) for b, o, d in rows]
    good, bad = fold(None), fold("body_offset_not_folded")
    par = np.array([g[0] for g in good])
    assert (par == [b[0] for b in bad]).all() and (np.diff(par) >= 0).all()
    as_rays = lambda rows: np.array([np.concatenate([o, d]) for _, o, d in rows]).astype(np.float32)
    ref = rc.reference_set(geom, q, box, as_rays(good), par)
    v = [rc.cast(geom, q[e], boxes[e], as_rays(bad), par, rc.MIN_RANGE, rc.MAX_RANGE) for e in range(N)]
    st = ~ref["unstable"]
    seg = np.stack([x["seg"] for x in v])
    same = st & (seg == ref["seg"]) & (seg != NONE)
    dp = np.abs(np.stack([x["point"] for x in v]) - ref["point"]).max(-1)
    found["body_offset_not_folded"] = (int((seg != ref["seg"])[st].sum()), {"point": float((dp[same] / rc.tolerances(ref)["p_abs"]).max())})
    print("variants miss their bound: " + "; ".join(f"{k}: {i} ids, " + ", ".join(f"{n} {x:.3g} x" for n, x in f.items()) for k, (i, f) in found.items()))
    assert set(found) == set(rc.VARIANTS)
    assert found["dir_not_rotated"][0] >= 20 and found["dir_not_rotated"][1]["normal"] >= 10
    assert found["min_range_ignored"][0] >= 20 and found["skip_ignored"][0] >= 20
    assert found["exit_hit"][1]["t"] >= 10
    assert found["body_offset_not_folded"][1]["point"] >= 10


def setup_hand():
    from dexrobot_isaac_amd.config import build_sim_config, default_cfg
    return build_sim_config(default_cfg("BlindGrasping"))[1]


# ------------------------------------------------------------------------------------------------- the user level on a stub core
_stub_core = stub_core(dict(raycast=lambda **kw: kw))


def test_env_level_arguments_folding_and_order():
    import torch
    from dexrobot_isaac_amd import make_env
    from oracle.py_backend import OracleCore
    env = make_env("BlindGrasping", 3, "cpu", "cpu", 0, _core_factory=_stub_core)
    o2, d2 = np.zeros((2, 3)), np.array([[0, 0, 1.0], [1.0, 0, 0]])
    bad = [
        (dict(origins=np.zeros((2, 2)), directions=d2), "shape"), (dict(origins=o2, directions=np.zeros((3, 3))), "shape"),
        (dict(origins=np.zeros(3), directions=np.ones(3)), "shape"),
        (dict(origins=np.zeros((0, 3)), directions=np.zeros((0, 3))), "between 1 and"),
        (dict(origins=np.zeros((_abi.RAY_MAX + 1, 3)), directions=np.ones((_abi.RAY_MAX + 1, 3))), "between 1 and"),
        (dict(origins=o2, directions=np.array([[0, 0, 1.0], [0, 0, 0]])), "zero"), (dict(origins=o2, directions=d2 * np.nan), "finite"),
        (dict(origins=o2, directions=d2, parent="no_such_link"), "unknown parent"), (dict(origins=o2, directions=d2, parent=NJ), "joint index"),
        (dict(origins=o2, directions=d2, parent=-1), "joint index"), (dict(origins=o2, directions=d2, parent=[5, 5, 5]), "one value or 2"),
        (dict(origins=o2, directions=d2, min_range=-0.1), "ranges"), (dict(origins=o2, directions=d2, min_range=0.5, max_range=0.5), "ranges"),
        (dict(origins=o2, directions=d2, max_range=float("inf")), "ranges"), (dict(origins=o2, directions=d2, max_range=float("nan")), "ranges"),
    ]
    for kw, text in bad:
        with pytest.raises(ValueError, match=text):
            env.create_ray_sensor("s", **kw)
    assert not env._ray_sensors and not env._core.calls
    # parents by index, DOF name, body name and None; a caller order that needs the unsort
    hand = env.model
    pad, mount = hand.body_names.index("r_f_link2_pad"), hand.body_names.index("hand_mount")
    origins = np.array([[0.0, 0.0, 0.002], [0.01, 0.0, 0.02], [0.5, 0.1, 0.9], [0.0, 0.0, 0.01], [0.003, 0.0, 0.0], [0.0, 0.0, 0.1]])
    dirs = np.array([[0.0, 0.0, 2.0], [0.0, 0.1, 1.0], [0.0, 0.0, -1.0], [0.1, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 0.0, -3.0]])
    parents = ["r_f_link2_pad", 5, None, "ARRz", "r_f_link1_4", "hand_mount"]
    env.create_ray_sensor("mixed", origins, dirs, parents, min_range=0.01, max_range=0.5, skip_parent=True)
    with pytest.raises(ValueError, match="already exists"):
        env.create_ray_sensor("mixed", origins, dirs, parents)
    res = env.read_ray_sensor("mixed", outputs=("dist", "hits"))
    kw = env._core.calls[-1]
    assert kw["parent"] == [-1, -1, 5, 5, 9, 13] and kw["skip_parent"] is True and abs(kw["min_range"] - 0.01) < 1e-12 and abs(kw["max_range"] - 0.5) < 1e-12
    assert kw["env_ids"] is None and kw["q"] is None and kw["box_pose"] is None and kw["box_size"] == 0.0
    assert kw["rays"].shape == (6, 6) and kw["rays"].dtype == torch.float32 and kw["dist"].shape == (3, 6) and kw["hits"].shape == (3, 6, 8)
    order = [2, 5, 1, 3, 4, 0]                                                 # the stable sort by parent of the caller's rays
    folded = [rc.fold_body(hand, pad, origins[0], dirs[0]), (5, origins[1], dirs[1]), (-1, origins[2], dirs[2]), (5, origins[3], dirs[3]),
              (hand.dof_names.index("r_f_joint1_4"), origins[4], dirs[4]), rc.fold_body(hand, mount, origins[5], dirs[5])]
    want = np.array([np.concatenate([folded[i][1], folded[i][2]]) for i in order])      # directions as given: the kernel normalises
    assert [folded[i][0] for i in order] == kw["parent"] and np.abs(kw["rays"].numpy() - want).max() <= 1e-7
    # ... and the folded ray is the body-frame ray: the same world ray through the reference's FK and the body's published pose
    geom = rr.HandGeometry(env._model_struct)
    q = np.random.default_rng(2).uniform(geom.lo, geom.hi)
    o, R = geom.fk(q)
    j, fo, fd = folded[0]
    body_o, body_R = o[j] + R[j] @ hand.body_p[pad], R[j] @ hand.body_R[pad]
    assert np.abs((o[j] + R[j] @ fo) - (body_o + body_R @ origins[0])).max() <= 1e-14 and np.abs(R[j] @ fd - body_R @ dirs[0]).max() <= 1e-14
    _, fo, fd = folded[5]                                                      # a body on the spawn frame folds to the world frame
    assert folded[5][0] == -1 and np.abs(fo - (hand.spawn_pos + hand.spawn_rot @ origins[5])).max() <= 1e-14
    # reads come back in the caller's order: column i of the result is column unsort[i] of what the kernel wrote
    kw["dist"].copy_(torch.arange(18.0).view(3, 6))
    kw["hits"].copy_(torch.arange(144.0).view(3, 6, 8))
    res = env.read_ray_sensor("mixed", outputs=("dist", "hits"), out={"dist": kw["dist"], "hits": kw["hits"]})
    inv = np.argsort(order)
    assert (res.dist.numpy() == np.arange(18.0).reshape(3, 6)[:, inv]).all() and (res.hits.numpy() == np.arange(144.0).reshape(3, 6, 8)[:, inv]).all()
    # a sorted sensor: the kernel's tensors as they are, `out` honoured, one parent for all
    env.create_ray_sensor("palm", origins[:2], dirs[:2], "ARRz")
    mine = torch.zeros(2, 2)
    res = env.read_ray_sensor("palm", env_ids=[2, 0], out={"dist": mine}, box_size=0.07)
    kw = env._core.calls[-1]
    assert res.dist is mine and res.hits is None and kw["dist"] is mine and "hits" not in kw and kw["parent"] == [5, 5]
    assert kw["env_ids"].tolist() == [2, 0] and abs(kw["box_size"] - 0.07) < 1e-12 and kw["skip_parent"] is False
    res = env.read_ray_sensor("palm", q=torch.zeros(5, NJ), box_pose=torch.zeros(5, 7), outputs="hits")
    assert res.dist is None and res.hits.shape == (5, 2, 8) and env._core.calls[-1]["box_pose"].shape == (5, 7)
    assert res.seg.dtype == torch.int32 and res.seg.shape == (5, 2) and res.points.shape == (5, 2, 3) and res.normals.shape == (5, 2, 3)
    assert [res.segment_name(i) for i in (NONE, GROUND, BOX)] == ["none", "ground", "box"]
    assert res.segment_name(CAP0) == res.segment_name(CAP0 + 2) == hand.body_names[6] and res.segment_name(CAP0 + 3 + 3 * 1 + 2) == "r_f_link2_4"
    with pytest.raises(IndexError):
        res.segment_name(CAP0 + NCAP)
    n_calls = len(env._core.calls)
    for kw, text in [(dict(outputs=()), "outputs"), (dict(outputs=("dist", "depth")), "outputs"), (dict(env_ids=[]), "empty"),
                     (dict(q=torch.zeros(3, NJ - 1)), "q must have shape"), (dict(box_pose=torch.zeros(3, 6)), "box_pose must have shape"),
                     (dict(box_size=0.0), "box_size"), (dict(box_size=float("nan")), "box_size"), (dict(out=[mine]), "out must be a dict"),
                     (dict(out={"hits": mine}), "out must be a dict"), (dict(out={"dist": torch.zeros(3, 3)}), "out must be a contiguous float32 tensor")]:
        with pytest.raises(ValueError, match=text):
            env.read_ray_sensor("palm", **kw)
    with pytest.raises(KeyError, match="no ray sensor"):
        env.read_ray_sensor("nope")
    assert len(env._core.calls) == n_calls                                     # nothing reached the core
    plain = make_env("BaseTask", 2, "cpu", "cpu", 0, _core_factory=OracleCore)   # the CPU stand-in has no ray caster
    with pytest.raises(NotImplementedError):
        plain.create_ray_sensor("s", o2, d2)
    with pytest.raises(NotImplementedError):
        plain.read_ray_sensor("s")


# ------------------------------------------------------------------------------------------------- GPU helpers
def _core(sc, ms, q, box=None):
    from dexrobot_isaac_amd.core import DexSimCore
    core = DexSimCore(sc, ms, "cuda:0")
    core.reset()
    pose_core(core, q, box)
    return core


@pytest.fixture(scope="module")
def rig(main):
    """A BlindGrasping core of N envs posed at the main set (hand and box), and its readings with and without skip_parent."""
    core = _core(main["sc"], main["ms"], main["q"], main["box"])
    full = {skip: rc.gpu_cast(core, N, main["rays"], main["parent"], skip_parent=skip) for skip in (False, True)}
    return dict(core=core, full=full)


def _against_reference(core, S, full=None):
    for skip in (False, True):
        dist, hits = full[skip] if full else rc.gpu_cast(core, N, S["rays"], S["parent"], skip_parent=skip)
        assert not np.isnan(dist).any() and not np.isnan(hits).any(), "an element was not written"
        rc.compare(S["refs"][skip], S["tols"][skip], dist, hits, f"skip_parent={skip}: ")
        d_alone, _ = rc.gpu_cast(core, N, S["rays"], S["parent"], skip_parent=skip, want=("dist",))
        _, h_alone = rc.gpu_cast(core, N, S["rays"], S["parent"], skip_parent=skip, want=("hits",))
        assert (bits(d_alone) == bits(dist)).all() and (bits(h_alone) == bits(hits)).all()       # each output alone: the same bits


# ------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_against_reference(rig, main):
    """Measured on one MI355X: see profiles/ray_sensors/README.md."""
    _against_reference(rig["core"], main, rig["full"])


@pytest.mark.gpu
def test_structure_free_model(main_generic):
    """The main comparison on the model of tests/generic_model.py, shares and bounds recomputed on its rows."""
    S = main_generic
    core = _core(S["sc"], S["ms"], S["q"], S["box"])
    _against_reference(core, S)
    core.close()


@pytest.mark.gpu
def test_chunking(rig, main):
    """R = 1, chunk - 1, chunk + 1 and a multiple of the chunk plus 3: every ray of a multi-chunk call equals, bit for bit, the same
    ray cast alone; so do the rays of the main set."""
    core, rays, parent = rig["core"], main["rays"], main["parent"]
    R = len(parent)
    assert R > 2 * CHUNK + 3
    alone = [rc.gpu_cast(core, N, rays[i:i + 1], parent[i:i + 1]) for i in range(R)]
    d1, h1 = np.concatenate([a[0] for a in alone], axis=1), np.concatenate([a[1] for a in alone], axis=1)
    assert (bits(d1) == bits(rig["full"][False][0])).all() and (bits(h1) == bits(rig["full"][False][1])).all()
    pick = np.sort(np.random.default_rng(7).permutation(R)[:2 * CHUNK + 3])
    for idx in (np.arange(CHUNK - 1), np.arange(R - CHUNK - 1, R), pick):
        d, h = rc.gpu_cast(core, N, rays[idx], parent[idx])
        assert (bits(d) == bits(d1[:, idx])).all() and (bits(h) == bits(h1[:, idx])).all(), len(idx)


@pytest.mark.gpu
def test_addressing(rig, main):
    import torch
    S, core = main, rig["core"]
    rays, parent, q, box = S["rays"], S["parent"], S["q"], S["box"]
    R = len(parent)
    dist, hits = rig["full"][False]
    # a permuted id list, k = 1, ids out of range
    ids = [69, 0, 64, 3, 63]
    d, h = rc.gpu_cast(core, len(ids), rays, parent, env_ids=ids)
    assert (bits(d) == bits(dist[ids])).all() and (bits(h) == bits(hits[ids])).all()
    d, h = rc.gpu_cast(core, 1, rays, parent, env_ids=[37])
    assert (bits(d) == bits(dist[[37]])).all() and (bits(h) == bits(hits[[37]])).all()
    ids = [5, -1, 69, N]
    d, h = rc.gpu_cast(core, len(ids), rays, parent, env_ids=ids)
    assert (bits(d[[0, 2]]) == bits(dist[[5, 69]])).all() and (bits(h[[0, 2]]) == bits(hits[[5, 69]])).all()
    assert np.isnan(d[[1, 3]]).all() and np.isnan(h[[1, 3]]).all()            # left as they were
    # 130 override rows (three workgroups): 70 equal to the state rows give the state path's bits, 60 are fresh
    g = np.random.default_rng(17)
    q2, box2 = rc.make_poses(S["geom"], 60, seed=rc.SEED + 1)
    qo, bo = np.concatenate([q, q2]), np.concatenate([box, box2])
    d, h = rc.gpu_cast(core, 130, rays, parent, q=qo, box=bo, env_ids=[-1])    # env_ids is ignored with an override
    assert (bits(d[:N]) == bits(dist)).all() and (bits(h[:N]) == bits(hits)).all()
    ref2 = rc.reference_set(S["geom"], q2, box2, rays, parent)
    assert ref2["unstable"].mean(1).max() <= MAX_UNSTABLE_ENV and ref2["unstable"].mean() <= MAX_UNSTABLE_ALL
    rc.compare(ref2, rc.tolerances(ref2), d[N:], h[N:], "60 fresh override rows: ")
    # a box_pose override on the state path, with another edge length; a q override without box_pose: no box
    perm = g.permutation(N)
    refb = rc.reference_set(S["geom"], q, box[perm], rays, parent, box_size=0.08)
    assert refb["unstable"].mean(1).max() <= MAX_UNSTABLE_ENV and refb["unstable"].mean() <= MAX_UNSTABLE_ALL
    d, h = rc.gpu_cast(core, N, rays, parent, box=box[perm], size=0.08)
    rc.compare(refb, rc.tolerances(refb), d, h, "box_pose and box_size override: ")
    refs = rc.reference_set(S["geom"], q, box, rays, parent, box_size=0.03)
    assert refs["unstable"].mean(1).max() <= MAX_UNSTABLE_ENV and refs["unstable"].mean() <= MAX_UNSTABLE_ALL
    d, h = rc.gpu_cast(core, N, rays, parent, size=0.03)
    rc.compare(refs, rc.tolerances(refs), d, h, "box_size override on the env's own box: ")
    refn = rc.reference_set(S["geom"], q, None, rays, parent)
    assert refn["unstable"].mean(1).max() <= MAX_UNSTABLE_ENV and refn["unstable"].mean() <= MAX_UNSTABLE_ALL
    d, h = rc.gpu_cast(core, N, rays, parent, q=q)
    assert not (bits(h[..., 7]) == BOX).any()
    rc.compare(refn, rc.tolerances(refn), d, h, "q override without a box: ")
    # argument errors that need a live handle launch nothing: the outputs stay NaN
    lib, h_ = core.lib, core.h
    out = torch.full((N, R), float("nan"), device=core.device)
    rp = torch.as_tensor(rays, device=core.device)
    par = (C.c_int * R)(*[int(p) for p in parent])
    op, rpp = C.c_void_p(out.data_ptr()), C.c_void_p(rp.data_ptr())
    call = lambda h=h_, k=N, parent=par, lo=0.0, hi=1.0, flags=0, size=0.0: lib.dexsim_raycast(h, None, k, None, None, size, rpp, parent, R, lo, hi, flags, op, None, None)
    assert call(k=N - 1) == 1 and b"k == num_envs" in lib.dexsim_last_error()
    assert call(parent=(C.c_int * R)(*[int(p) for p in parent[::-1]])) == 1 and call(lo=0.5, hi=0.1) == 1 and call(flags=4) == 1
    h2 = C.c_void_p()
    assert lib.dexsim_create(C.byref(S["sc"]), C.byref(S["ms"]), core.dev_index, C.byref(h2)) == 0
    assert call(h=h2) == 2                                                     # DEXSIM_ERR_NOT_BOUND
    assert lib.dexsim_destroy(h2) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any())


@pytest.mark.gpu
def test_no_box_task(main):
    """A BaseTask core has no box: no ray reports one on the state path; a box_pose override brings one in."""
    S = main
    sc, ms = setup(N, "BaseTask")
    assert not sc.has_box
    core = _core(sc, ms, S["q"])
    refn = rc.reference_set(S["geom"], S["q"], None, S["rays"], S["parent"])
    d, h = rc.gpu_cast(core, N, S["rays"], S["parent"])
    assert not (bits(h[..., 7]) == BOX).any()
    rc.compare(refn, rc.tolerances(refn), d, h, "BaseTask: ")
    d, h = rc.gpu_cast(core, N, S["rays"], S["parent"], box=S["box"], size=rc.BOX_SIZE)
    rc.compare(S["refs"][False], S["tols"][False], d, h, "BaseTask with a box_pose override: ")
    core.close()


@pytest.mark.gpu
def test_contract_with_the_camera(rig, main):
    """The rays of a small world camera -- 8 x 6 pixel directions from render_ref.pixel_rays, a wide clip window -- give the
    camera's segmentation exactly on the pixels stable for both, and t cos matches its depth within the two derived tolerances."""
    import torch
    S, core = main, rig["core"]
    W, H, hfov, near, far = 8, 6, 60.0, 1e-3, 10.0
    cen = S["box"][:, :3].mean(0).astype(np.float64)
    eye, target = (cen + [0.26, -0.12, 0.2]).astype(np.float32), (cen + [0.0, 0.0, 0.03]).astype(np.float32)
    cam = rr.look_at(eye.astype(np.float64), target.astype(np.float64))
    dirs, _ = rr.pixel_rays(cam, W, H, hfov)
    rays = np.concatenate([np.tile(eye, (W * H, 1)), dirs.astype(np.float32)], axis=1)
    cosax = rr._unit(rays[:, 3:].astype(np.float64)) @ cam[3]
    parent = np.full(W * H, -1)
    boxes = [(S["box"][e, :3].astype(np.float64), S["box"][e, 3:].astype(np.float64), rc.BOX_SIZE) for e in range(N)]
    imgs = [rr.render_with_stability(S["geom"], S["q"][e], boxes[e], cam, W, H, hfov, near, far) for e in range(N)]
    ref = rc.reference_set(S["geom"], S["q"], S["box"], rays, parent, min_range=0.0, max_range=20.0)
    stable = ~ref["unstable"] & ~np.stack([i["unstable"].ravel() for i in imgs])
    print(f"{stable.mean():.3f} of the pixels are stable for both")
    assert stable.mean() >= 0.9 and (ref["seg"] == np.stack([i["seg"].ravel() for i in imgs]))[stable].all()
    c = _abi.DexSimCamera()
    c.width, c.height, c.hfov_deg, c.near_clip, c.far_clip, c.parent_joint = W, H, hfov, near, far, -1
    for i in range(3):
        c.eye[i], c.target[i] = float(eye[i]), float(target[i])
    scene = torch.zeros(N, core.render_layout()[1], device=core.device)
    depth, seg = torch.zeros(N, H, W, device=core.device), torch.zeros(N, H, W, dtype=torch.int32, device=core.device)
    core.render(c, scene, depth=depth, seg=seg)
    torch.cuda.synchronize()
    depth, seg = depth.cpu().numpy().reshape(N, -1), seg.cpu().numpy().reshape(N, -1)
    d, h = rc.gpu_cast(core, N, rays, parent, min_range=0.0, max_range=20.0)
    assert (bits(h[..., 7]) == seg)[stable].all()
    # each side is within ten times its own reference's float32 error of the float64 truth
    tol = rc.tolerances(ref)
    e_abs, e_rel = 0.0, 0.0
    for i in imgs:
        ok = ~i["unstable"] & (i["seg32"] == i["seg"]) & (i["seg"] != NONE)
        err = np.abs(np.where(ok, i["depth32"].astype(np.float64), 0) - np.where(ok, i["depth"], 0))
        gnd = ok & (i["seg"] == GROUND)
        e_abs = max(e_abs, err[ok & ~gnd].max(initial=0))
        e_rel = max(e_rel, (err[gnd] / i["depth"][gnd]).max(initial=0))
    hit = stable & (ref["seg"] != NONE)
    gnd, obj = hit & (ref["seg"] == GROUND), hit & (ref["seg"] != GROUND)
    diff = np.abs(np.where(hit, d.astype(np.float64) * cosax[None, :], 0) - np.where(hit, depth.astype(np.float64), 0))
    scale = np.where(hit, ref["t"] * cosax[None, :], 1.0)
    b_abs, b_rel = 10 * e_abs + tol["t_abs"], 10 * e_rel + tol["t_rel"]
    print(f"t cos against the camera's depth: {diff[obj].max():.3g} m on hand and box hits (bound {b_abs:.3g}), "
          f"{(diff / scale)[gnd].max():.3g} relative on the ground (bound {b_rel:.3g})")
    assert diff[obj].max() <= b_abs and (diff / scale)[gnd].max() <= b_rel


@pytest.mark.gpu
def test_fingertip_rays_read_the_site_height(main):
    """A world ray straight down from a fingertip site reads the z of get_site_poses wherever it reports the ground."""
    import torch
    from dexrobot_isaac_amd import make_env
    S = main
    env = make_env("BlindGrasping", N, "cuda:0", "cuda:0", 0)
    env.reset()
    pose_core(env._core, S["q"], S["box"])
    tips = env.get_site_poses("tips")[..., :3].cpu().numpy()                   # (N, 5, 3)
    seen, worst = 0, 0.0
    for e in (0, 3, 17, 31, 42, 55, 63, 64, 69):
        rays = np.concatenate([tips[e], np.tile([0.0, 0.0, -1.0], (5, 1))], axis=1).astype(np.float32)
        d, h = rc.gpu_cast(env._core, 1, rays, [-1] * 5, env_ids=[e], min_range=0.0, max_range=1.0)
        gnd = bits(h[0, :, 7]) == GROUND
        seen += int(gnd.sum())
        if gnd.any():
            worst = max(worst, float((np.abs(d[0][gnd].astype(np.float64) - tips[e][gnd, 2]) / tips[e][gnd, 2]).max()))
            assert (np.abs(h[0][gnd, 1:3] - tips[e][gnd, :2]) <= 1e-6).all() and (np.abs(h[0][gnd, 3]) <= 1e-6).all()
    print(f"{seen} rays see the ground, t off the site height by {worst:.3g} relative (bound {S['tols'][False]['t_rel']:.3g})")
    assert seen >= 5 and worst <= S["tols"][False]["t_rel"]
    env.close()


@pytest.mark.gpu
def test_purity_and_determinism(main):
    S = main
    calls = lambda core: list(rc.gpu_cast(core, N, S["rays"], S["parent"], skip_parent=True))

    def between(core):
        rc.gpu_cast(core, 3, S["rays"][:5], S["parent"][:5], env_ids=[4, 66, 1], want=("dist",))
        rc.gpu_cast(core, 9, S["rays"], S["parent"], q=S["q"][:9], box=S["box"][:9], size=0.07, min_range=0.0)
    dist, hits = purity_frame(calls, between)
    assert not np.isnan(dist).any() and not np.isnan(hits).any() and (bits(hits[..., 7]) != NONE).any()


@pytest.mark.gpu
def test_public_surface(rig, main):
    """Sensors through make_env: body names, a caller order that needs the unsort, segment_name, out=."""
    import torch
    from dexrobot_isaac_amd import make_env
    S = main
    env = make_env("BlindGrasping", N, "cuda:0", "cuda:0", 0)
    env.reset()
    pose_core(env._core, S["q"], S["box"])
    hand = env.model
    rows = _body_rays(hand)
    rows = rows[::-1]                                                          # pinky first: the caller's order is not the parents'
    names = [hand.body_names[b] for b, _, _ in rows]
    env.create_ray_sensor("skin", [o for _, o, _ in rows], [d for _, _, d in rows], names, min_range=rc.MIN_RANGE, max_range=rc.MAX_RANGE)
    res = env.read_ray_sensor("skin", outputs=("dist", "hits"))
    torch.cuda.synchronize()
    folded = [rc.fold_body(hand, b, o, d) for b, o, d in rows]
    rays = np.array([np.concatenate([o, d]) for _, o, d in folded]).astype(np.float32)
    par = np.array([j for j, _, _ in folded])
    assert (np.diff(par) < 0).any()
    order = np.argsort(par, kind="stable")
    inv = np.argsort(order)
    ref = rc.reference_set(S["geom"], S["q"], S["box"], rays[order], par[order])
    assert ref["unstable"].mean(1).max() <= MAX_UNSTABLE_ENV and ref["unstable"].mean() <= MAX_UNSTABLE_ALL
    ref = {k: v[:, inv] for k, v in ref.items()}                               # the reference in the caller's order
    dist, hits = res.dist.cpu().numpy(), res.hits.cpu().numpy()
    rc.compare(ref, rc.tolerances(ref), dist, hits, "sensors on body names: ")
    seg = res.seg.cpu().numpy()
    assert (seg == bits(hits[..., 7])).all() and torch.equal(res.points, res.hits[..., 1:4]) and torch.equal(res.normals, res.hits[..., 4:7])
    c = int(seg[seg >= CAP0][0])
    assert res.segment_name(c) == hand.body_names[[int(s) for s in hand.body_fslot].index(int(hand.cap_fslot[c - CAP0]))]
    # a sorted sensor with out=: the caller's tensor is what the kernel wrote and what is returned; ids out of range stay as they were
    env.create_ray_sensor("main", S["rays"][:, :3], S["rays"][:, 3:], [None if p < 0 else int(p) for p in S["parent"]],
                          min_range=rc.MIN_RANGE, max_range=rc.MAX_RANGE)
    mine = torch.full((3, len(S["parent"])), -5.0, device=env._core.device)
    res = env.read_ray_sensor("main", env_ids=[69, N, 0], out={"dist": mine})
    torch.cuda.synchronize()
    assert res.dist is mine and res.hits is None
    got = mine.cpu().numpy()
    assert (bits(got[[0, 2]]) == bits(rig["full"][False][0][[69, 0]])).all() and (got[1] == -5.0).all()
    res = env.read_ray_sensor("main", env_ids=[N, 2])
    torch.cuda.synchronize()
    assert bool(torch.isnan(res.dist[0]).all()) and (bits(res.dist[1].cpu().numpy()) == bits(rig["full"][False][0][2])).all()
    env.close()
