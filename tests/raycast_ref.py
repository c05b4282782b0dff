"""Reference for the range sensors (include/dexsim_ray.h, a part of dexsim.h; dexsim_raycast): the specification the GPU kernel is tested
against.  Plain numpy, float64 by default; every function takes `dtype` so that the SAME code can be evaluated in float32 -- the
tolerances of tests/test_raycast.py are ten times the error this reference makes in float32, the rule of tests/test_render.py.

The intersection rule is the camera's, and tests/render_ref.py is its written specification: HandGeometry (forward kinematics from
the header's joint-frame formula and the DexHandModel numbers), ray_capsule, ray_box and quat_to_mat are taken from there.  Those
primitives cast many rays from ONE origin; a sensor's rays each have their own, so ray_capsules / ray_boxes below are the same
formulas with an origin per ray (test_raycast.test_reference_primitives holds them against render_ref's on shared origins).  This
module adds what a range sensor has and a camera has not: per-ray origins, parent frames from HandGeometry.fk, the folding of a body
frame into its joint frame from the HandModel numbers, the range window, the skip flag, the hit point and the normal.

It also marks the rays whose answer is not defined at float32 resolution ("unstable", left out of comparisons), by the criteria of
render_ref:
  (a) the id changes when every primitive is inflated or deflated by MARGIN = 0.2 mm (capsule radii, box half-extent, ground height);
  (b) a box hit within MARGIN of a box edge, in box coordinates: the normal is discontinuous there;
  (c) t is within 1e-3 relative of min_range or max_range;
  (d) a GROUND hit by a ray with |d_z| < 1e-3.
"""
import numpy as np

from dexrobot_isaac_amd import _abi
from tests import render_ref as rr

MARGIN = rr.MARGIN
VARIANTS = ("dir_not_rotated", "body_offset_not_folded", "min_range_ignored", "skip_ignored", "exit_hit")


# ------------------------------------------------------------------------------------------------- primitives, an origin per ray
def _root(b, c, sign):
    """Root -b + sign sqrt(b^2 - c) of t^2 + 2 b t + c = 0 (inf where there is none); sign = -1: the entering one."""
    h = b * b - c
    with np.errstate(invalid="ignore"):
        return np.where(h >= 0, -b + sign * np.sqrt(np.maximum(h, 0)), np.inf)


def ray_capsules(ro, rd, a, b, r, exit_hit=False):
    """render_ref.ray_capsule with origins ro (P, 3): t (P,) of the entering hit (inf = miss) and outward unit normals (P, 3).
    exit_hit: the leaving root of every quadratic instead (a deliberate mistake for the discrimination test)."""
    dt = rd.dtype
    sign = dt.type(1 if exit_hit else -1)
    ba = b - a
    L = np.sqrt((ba * ba).sum())
    u = ba / L
    o = ro - a
    ud, uo = rd @ u, o @ u
    rp, op = rd - ud[:, None] * u, o - uo[:, None] * u
    A, B, C = (rp * rp).sum(-1), (rp * op).sum(-1), (op * op).sum(-1) - r * r
    h = B * B - A * C
    with np.errstate(invalid="ignore", divide="ignore"):
        tb = np.where((h >= 0) & (A > 1e-12), (-B + sign * np.sqrt(np.maximum(h, 0))) / np.where(A > 1e-12, A, 1), np.inf)
        yb = uo + np.where(np.isfinite(tb), tb, 0) * ud
    tb = np.where((yb > 0) & (yb < L), tb, np.inf)
    ob = ro - b
    ta = _root((rd * o).sum(-1), (o * o).sum(-1) - r * r, sign)
    tc = _root((rd * ob).sum(-1), (ob * ob).sum(-1) - r * r, sign)
    t = np.minimum(tb, np.minimum(ta, tc))
    y = np.where(t == tb, yb, np.where(t == ta, 0, L)).astype(dt)
    ts = np.where(np.isfinite(t), t, 0).astype(dt)
    n = (o + ts[:, None] * rd - y[:, None] * u[None, :]) / r
    return t.astype(dt), n.astype(dt)


def ray_boxes(ro, rd, c, R, half, exit_hit=False):
    """render_ref.ray_box with origins ro (P, 3): t, outward normals (world) and the hit points in box coordinates."""
    dt = rd.dtype
    ob, db = (ro - c) @ R, rd @ R
    db = np.where(np.abs(db) > 1e-30, db, dt.type(1e-30))
    m = 1 / db
    t1, t2 = -ob * m - np.abs(m) * half, -ob * m + np.abs(m) * half
    tn, tf = t1.max(-1), t2.min(-1)
    ax = t2.argmin(-1) if exit_hit else t1.argmax(-1)
    rows = np.arange(len(ax))
    t = np.where(tn <= tf, tf if exit_hit else tn, np.inf)
    nb = np.zeros_like(db)
    nb[rows, ax] = (1 if exit_hit else -1) * np.sign(db[rows, ax])
    pl = ob + np.where(np.isfinite(t), t, 0)[:, None] * db
    return t.astype(dt), (nb @ R.T).astype(dt), pl


# ------------------------------------------------------------------------------------------------- frames
def fold_body(hand, body, origin, direction, variant=None):
    """A ray given in the frame of hand body `body` (an index into hand_model.BODY_NAMES) as a ray in the joint frame the body is
    welded to, from the HandModel numbers body_parent / body_p / body_R, in float64: (joint or -1, origin, direction).  A body on
    the spawn frame (body_parent -1) folds to the world frame through the spawn pose."""
    Rb, pb = np.asarray(hand.body_R[body], dtype=np.float64), np.asarray(hand.body_p[body], dtype=np.float64)
    o, d = np.asarray(origin, dtype=np.float64), np.asarray(direction, dtype=np.float64)
    if variant == "body_offset_not_folded":
        pb = np.zeros(3)
    o, d = pb + Rb @ o, Rb @ d
    j = int(hand.body_parent[body])
    if j < 0:
        o, d = np.asarray(hand.spawn_pos, dtype=np.float64) + hand.spawn_rot @ o, hand.spawn_rot @ d
    return j, o, d


def world_rays(geom, q, rays, parent, dtype=np.float64, variant=None):
    """The rays (R, 6) -- origin and direction in the frame parent[i] (-1: world, else a joint) -- in world coordinates at joint
    positions q: origins (R, 3), unit directions (R, 3), `live` (R,) bool (|d|^2 >= 1e-24), and the joint frames."""
    dt = np.dtype(dtype)
    o, R = geom.fk(np.asarray(q, dtype=np.float64).astype(dt), dtype)
    po, pd = rays[:, :3].astype(dt), rays[:, 3:].astype(dt)
    n2 = (pd * pd).sum(-1)
    live = n2 >= 1e-24
    du = pd / np.sqrt(np.where(live, n2, 1))[:, None]
    ro, rd = po.copy(), du.copy()
    for i, j in enumerate(parent):
        if j >= 0:
            ro[i] = o[j] + R[j] @ po[i]
            rd[i] = du[i] if variant == "dir_not_rotated" else R[j] @ du[i]
    return ro.astype(dt), rd.astype(dt), live, (o, R)


# ------------------------------------------------------------------------------------------------- the cast
def cast(geom, q, box, rays, parent, min_range=0.0, max_range=1.0, skip_parent=False, dtype=np.float64, inflate=0.0, variant=None):
    """The readings of one env.  box = (pos (3,), quat xyzw (4,), size) or None; rays (R, 6), parent (R,) ints.  Returns a dict:
    t (R,) (inf without a hit), seg (R,) int32, point (R, 3), normal (R, 3) (zeros without a hit), box_edge (R,) bool (criterion
    b), dz (R,) the z component of the unit direction."""
    dt = np.dtype(dtype)
    T = dt.type
    parent = np.asarray(parent)
    a, b, _ = geom.capsules(np.asarray(q, dtype=np.float64).astype(dt), dtype)
    ro, rd, live, _ = world_rays(geom, q, rays, parent, dtype, variant)
    P = len(parent)
    lo = T(0.0 if variant == "min_range_ignored" else min_range)
    hi = T(max_range)
    best = np.full(P, np.inf, dtype=dt)
    seg = np.zeros(P, dtype=np.int32)
    nrm = np.zeros((P, 3), dtype=dt)
    edge = np.zeros(P, dtype=bool)
    ex = variant == "exit_hit"

    def take(t, n, sid, allowed=True, e=None):
        nonlocal best, seg, nrm, edge
        with np.errstate(invalid="ignore"):
            ok = live & allowed & (t >= lo) & (t <= hi) & (t < best)
        best = np.where(ok, t, best)
        seg = np.where(ok, sid, seg).astype(np.int32)
        nrm = np.where(ok[:, None], n, nrm)
        edge = np.where(ok, e if e is not None else False, edge)

    dz = np.where(np.abs(rd[:, 2]) > 1e-30, rd[:, 2], T(1e-30))
    up = np.zeros((P, 3), dtype=dt)
    up[:, 2] = 1
    take(-(ro[:, 2] - T(inflate)) / dz, up, _abi.SEG_GROUND)
    if box is not None:
        half = T(0.5 * float(box[2]) + inflate)
        Rb = rr.quat_to_mat(box[1], dtype)
        t, n, pl = ray_boxes(ro, rd, np.asarray(box[0], dtype=np.float64).astype(dt), Rb, half, ex)
        near_face = (np.abs(half - np.abs(pl)) < MARGIN).sum(-1)
        take(t, n, _abi.SEG_BOX, True, near_face >= 2)
    skip = bool(skip_parent) and variant != "skip_ignored"
    for c in range(_abi.NCAP):
        t, n = ray_capsules(ro, rd, a[c], b[c], T(geom.cap_r[c] + inflate), ex)
        allowed = ~((parent >= 0) & (parent == geom.cap_parent[c])) if skip else True
        take(t, n, _abi.SEG_CAPSULE0 + c, allowed)
    hit = seg != _abi.SEG_NONE
    point = np.where(hit[:, None], ro + np.where(hit, best, 0)[:, None] * rd, 0).astype(dt)
    return {"t": best, "seg": seg, "point": point, "normal": np.where(hit[:, None], nrm, 0).astype(dt), "box_edge": edge, "dz": rd[:, 2]}


def cast_with_stability(geom, q, box, rays, parent, min_range=0.0, max_range=1.0, skip_parent=False):
    """float64 readings plus `unstable` (R,) bool -- criteria (a)-(d) of the module docstring -- and the readings of the same
    reference evaluated in float32 under "f32"."""
    kw = dict(min_range=min_range, max_range=max_range, skip_parent=skip_parent)
    out = cast(geom, q, box, rays, parent, **kw)
    up = cast(geom, q, box, rays, parent, inflate=+MARGIN, **kw)
    dn = cast(geom, q, box, rays, parent, inflate=-MARGIN, **kw)
    t = out["t"]
    with np.errstate(invalid="ignore"):
        window = np.isfinite(t) & ((np.abs(t - min_range) <= 1e-3 * min_range) | (np.abs(t - max_range) <= 1e-3 * max_range))
    horizon = (out["seg"] == _abi.SEG_GROUND) & (np.abs(out["dz"]) < 1e-3)
    out["unstable"] = (up["seg"] != out["seg"]) | (dn["seg"] != out["seg"]) | out["box_edge"] | window | horizon
    out["f32"] = cast(geom, q, box, rays, parent, dtype=np.float32, **kw)
    return out


# ------------------------------------------------------------------------------------------------- the test set
ROWS, SEED, BOX_SIZE = 70, 31, 0.05
MIN_RANGE, MAX_RANGE = 0.03, 1.0


def make_poses(geom, n=ROWS, box_size=BOX_SIZE, seed=SEED):
    """The pose recipe of the camera tests, restated: hand lowered by q[2] = -0.2 (fingertips ~0.10 m above the ground), finger
    joints uniform over their ranges, base rotations +-0.25 rad; box within +-3 cm of the capsule centroid, 0-3 cm above rest,
    random orientation.  Everything is rounded to float32, which is what both sides are given.  Returns q (n, 26), box (n, 7)."""
    rng = np.random.default_rng(seed)
    q = np.zeros((n, _abi.NJ))
    q[:, 0:2] = rng.uniform(-0.02, 0.02, (n, 2))
    q[:, 2] = -0.2
    q[:, 3:6] = rng.uniform(-0.25, 0.25, (n, 3))
    q[:, 6:] = rng.uniform(geom.lo[6:], geom.hi[6:], (n, 20))
    q = q.astype(np.float32)
    box = np.zeros((n, 7))
    for e in range(n):
        a, b, _ = geom.capsules(q[e].astype(np.float64))
        cen = (0.5 * (a + b)).mean(0)
        box[e, :3] = [cen[0] + rng.uniform(-0.03, 0.03), cen[1] + rng.uniform(-0.03, 0.03), 0.5 * box_size + rng.uniform(0, 0.03)]
        box[e, 3:] = rr._unit(rng.normal(size=4))
    return q, box.astype(np.float32)


def make_rays(ms, box_mean):
    """The main ray set (R, 6) float32 and its parents (R,), sorted by parent: four rays from every fingertip site and three from
    every pad site on the distal joint frames; a 4 x 4 fan up from the palm frame (along its normal) and one down (along the fingers); three rays from 6 cm above the palm
    capsules and one from 5 cm above every distal link pointing back through them (what skip_parent changes); twelve world rays from
    above and from the side aimed at the mean box position `box_mean`, none within 1e-2 of horizontal."""
    site_p = np.array(np.ctypeslib.as_array(ms.site_p), dtype=np.float64)
    Rm = rr.quat_to_mat(np.array(np.ctypeslib.as_array(ms.site_q), dtype=np.float64)[0])    # palm frame: x fingers, y across, z normal
    cap1 = np.array(np.ctypeslib.as_array(ms.cap_p1), dtype=np.float64)
    cap0 = np.array(np.ctypeslib.as_array(ms.cap_p0), dtype=np.float64)
    rows = []                                                                  # (parent, origin, direction)
    for f in range(_abi.NFINGER):
        jd = 9 + 4 * f
        for d in ([1, 0, 0], [1, 0, 0.5], [1, 0, -0.5], [1, 0.5, 0.2]):
            rows.append((jd, site_p[1 + f], d))
        for d in ([0, 0, 1], [0.4, 0, 1], [-0.4, 0.3, 1]):
            rows.append((jd, site_p[6 + f], d))
        c = 3 + 3 * f + 2                                                      # the distal capsule: from 5 cm off its middle, back through it
        mid = 0.5 * (cap0[c] + cap1[c])
        rows.append((jd, mid + [0, 0, 0.05], [0.02, 0.01, -1]))
    grid = (-0.6, -0.2, 0.2, 0.6)
    for sx in grid:                                                            # along the palm normal, over the curling fingers
        for sy in grid:
            rows.append((5, Rm @ [0.05, 0.0, 0.02], Rm @ [sx, sy, 1.0]))
    for sy in grid:                                                            # along the fingers, from the palm side: towards the box and the ground
        for sz in grid:
            rows.append((5, Rm @ [0.05, 0.0, 0.03], Rm @ [1.0, 0.5 * sy, 0.5 * sz - 0.1]))
    for y in (-0.026, 0.0, 0.026):
        rows.append((5, Rm @ [0.05, y, 0.06], Rm @ [0.01, 0.02, -1]))
    bm = np.asarray(box_mean, dtype=np.float64)
    for k, (dx, dy) in enumerate(((0.0, 0.0), (0.02, -0.01), (-0.015, 0.02), (0.03, 0.03))):
        o = bm + [0.05 * (k - 1.5), 0.04 * (1.5 - k), 0.4]
        rows.append((-1, o, bm + [dx, dy, 0.0] - o))
    for k, az in enumerate((0.3, 1.9, 3.5, 5.1, 1.1, 2.7, 4.3, 5.9)):
        o = bm + [0.3 * np.cos(az), 0.3 * np.sin(az), (0.12 + 0.03 * k) if k < 4 else (0.03 + 0.015 * k)]
        rows.append((-1, o, bm + [0.0, 0.0, 0.01 * (k % 4)] - o))
    parent = np.array([r[0] for r in rows])
    order = np.argsort(parent, kind="stable")
    rays = np.array([np.concatenate([np.asarray(r[1], dtype=np.float64), np.asarray(r[2], dtype=np.float64)]) for r in rows])
    return rays[order].astype(np.float32), parent[order]


def reference_set(geom, q, box, rays, parent, box_size=BOX_SIZE, min_range=MIN_RANGE, max_range=MAX_RANGE, skip_parent=False):
    """cast_with_stability of every row, stacked: t, seg, point, normal, unstable (n, R, ...) and t32, seg32, point32, normal32."""
    rows = [cast_with_stability(geom, q[e], None if box is None else (box[e, :3], box[e, 3:], box_size), rays, parent, min_range,
                                max_range, skip_parent) for e in range(len(q))]
    out = {k: np.stack([r[k] for r in rows]) for k in ("t", "seg", "point", "normal", "unstable")}
    for k in ("t", "seg", "point", "normal"):
        out[k + "32"] = np.stack([r["f32"][k] for r in rows])
    return out


def tolerances(ref, factor=10.0):
    """Ten times the float32 error of the reference on its stable rays, per quantity: "t_abs" (hand and box hits, metres), "t_rel"
    (ground hits), "p_abs", "p_rel" (hit point: absolute on hand and box hits, relative to t on the ground), "n" (normal
    components); and the measured errors themselves under "err"."""
    ok = ~ref["unstable"] & (ref["seg32"] == ref["seg"]) & (ref["seg"] != _abi.SEG_NONE)
    gnd, obj = ok & (ref["seg"] == _abi.SEG_GROUND), ok & (ref["seg"] != _abi.SEG_GROUND)
    t64 = np.where(ok, ref["t"], 1.0)
    dt = np.abs(np.where(ok, ref["t32"].astype(np.float64), 1.0) - t64)
    dp = np.abs(ref["point32"].astype(np.float64) - ref["point"]).max(-1)
    dn = np.abs(ref["normal32"].astype(np.float64) - ref["normal"]).max(-1)
    err = {"t_abs": float(dt[obj].max()), "t_rel": float((dt / t64)[gnd].max()), "p_abs": float(dp[obj].max()),
           "p_rel": float((dp / t64)[gnd].max()), "n": float(dn[ok].max())}
    tol = {k: factor * v for k, v in err.items()}
    tol["err"] = err
    tol["mismatch32"] = int((ref["seg32"] != ref["seg"])[~ref["unstable"]].sum())
    return tol


def compare(ref, tol, t, hits=None, what=""):
    """A result (dist `t` (n, R) and / or `hits` (n, R, 8), numpy) against the reference on its stable rays: ids exact, t, point and
    normal within `tol`; the record's own rules (no hit: +inf, zeros, SEG_NONE).  Returns the measured errors."""
    st = ~ref["unstable"]
    hit = ref["seg"] != _abi.SEG_NONE
    gnd, obj = st & (ref["seg"] == _abi.SEG_GROUND), st & hit & (ref["seg"] != _abi.SEG_GROUND)
    m = {}
    if hits is not None:
        seg = np.ascontiguousarray(hits[..., 7]).view(np.int32)
        bad = int((seg != ref["seg"])[st].sum())
        assert bad == 0, f"{what}{bad} of {int(st.sum())} stable rays have another segment id"
        if t is not None:
            assert (np.ascontiguousarray(t).view(np.int32) == np.ascontiguousarray(hits[..., 0]).view(np.int32)).all(), f"{what}dist differs from word 0 of hits"
        t = hits[..., 0]
        none = seg == _abi.SEG_NONE
        assert np.isposinf(hits[..., 0][none]).all() and (np.ascontiguousarray(hits[..., 1:7][none]).view(np.int32) == 0).all(), f"{what}a no-hit record"
        assert np.isfinite(hits[~none]).all()
        p, n = hits[..., 1:4].astype(np.float64), hits[..., 4:7].astype(np.float64)
        dp, dn = np.abs(p - ref["point"]).max(-1), np.abs(n - ref["normal"]).max(-1)
        t64 = np.where(hit, ref["t"], 1.0)
        m["p_abs"], m["p_rel"], m["n"] = float(dp[obj].max()), float((dp / t64)[gnd].max()), float(dn[st & hit].max())
        assert np.abs(np.linalg.norm(n[~none], axis=-1) - 1).max() <= 1e-5
    t = t.astype(np.float64)
    assert (np.isposinf(t) == ~hit)[st].all(), f"{what}hit / no hit differs on a stable ray"
    t64 = np.where(hit, ref["t"], 1.0)
    dt = np.abs(np.where(hit & np.isfinite(t), t, 1.0) - t64)
    m["t_abs"], m["t_rel"] = float(dt[obj].max()), float((dt / t64)[gnd].max())
    print(what + "measured against float64: " + ", ".join(f"{k} {v:.3g} (bound {tol[k]:.3g})" for k, v in sorted(m.items())))
    for k, v in m.items():
        assert v <= tol[k], f"{what}{k}: {v:.3g} above the bound {tol[k]:.3g}"
    return m


# ------------------------------------------------------------------------------------------------- the device call
def gpu_cast(core, k, rays, parent, env_ids=None, q=None, box=None, size=0.0, min_range=MIN_RANGE, max_range=MAX_RANGE, skip_parent=False,
             want=("dist", "hits")):
    """core.raycast into guarded outputs: (dist, hits) as numpy arrays, None where not asked."""
    import torch
    from tests.query_rig import GUARD, guarded, guards_ok
    R = len(parent)
    bufs = {}
    if "hits" in want:
        bufs["hits"] = guarded(k, R, 8)
    if "dist" in want:   # a guard row of R words would leave the rows behind it off the 16-byte alignment the call asks for: 64 words
        flat = torch.full((k * R + 128,), float("nan"), dtype=torch.float32, device="cuda:0")
        flat[:64], flat[-64:] = GUARD, GUARD
        bufs["dist"] = (flat, flat[64:-64].view(k, R))
    dev = lambda x: None if x is None else torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device=core.device)
    core.raycast(rays=dev(rays), parent=[int(p) for p in parent], env_ids=env_ids, q=dev(q), box_pose=dev(box), box_size=size,
                 min_range=min_range, max_range=max_range, skip_parent=skip_parent, **{o: v for o, (_, v) in bufs.items()})
    if "hits" in want:
        guards_ok(bufs["hits"][0])
    if "dist" in want:
        torch.cuda.synchronize()
        flat = bufs["dist"][0]
        assert bool((flat[:64] == GUARD).all()) and bool((flat[-64:] == GUARD).all()), "a guard word of dist was written"
    out = {o: v.cpu().numpy() for o, (_, v) in bufs.items()}
    return out.get("dist"), out.get("hits")
