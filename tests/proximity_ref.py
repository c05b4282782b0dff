"""Reference for the clearance queries (include/dexsim.h, "clearance queries"): a numpy statement of the header's geometry on top of
render_ref.HandGeometry.capsules, the forward kinematics the render tests already pin against the engine's geometry.  Every function
takes `dtype`: float64 is the reference, float32 the same code at the device's precision -- the tolerances of tests/test_proximity.py
are 4 x the difference of the two on the test's own rows.  It shares no code with the engine.  Vectorised over rows (only the
forward kinematics loops over them).

The capsule / box minimiser is found here by SORTING the candidates (0, 1 and the six clamped breakpoints of f') and interpolating f'
on the first piece where it turns non-negative; the kernel brackets the same piece without sorting.
tests/test_proximity.py::test_reference_against_brute_force holds both segment routines against a dense sampling.
"""
import numpy as np

from dexrobot_isaac_amd import _abi
from tests.query_rig import bits, guarded, guards_ok
from tests.render_ref import HandGeometry, quat_to_mat

NCAP, NGROUP, NPAIR = _abi.NCAP, _abi.NPROX_GROUPS, _abi.NPROX_PAIRS
FINGER_PAIRS = [(a, b) for a in range(5) for b in range(a + 1, 5)]
MEET = 1e-6          # axis distance at or below which the axis "meets" the box (the header's threshold)
ZERO_AXIS2 = 1e-18   # |axis|^2 at or below which a capsule is a sphere
PARALLEL = 1e-12


def pair_table():
    """The header's pair table: (capsule A, capsule B, group) of the 120 pairs.  Capsule 3 + 3 f + l is link l of finger f."""
    out = []
    for g, (fa, fb) in enumerate(FINGER_PAIRS):
        out += [(3 + 3 * fa + la, 3 + 3 * fb + lb, g) for la in range(3) for lb in range(3)]
    for f in range(5):
        out += [(i, 3 + 3 * f + lb, 10 + f) for i in range(3) for lb in (1, 2)]
    return out


def _dot(a, b):
    return (a * b).sum(-1)


def _clip01(x):
    return np.minimum(np.maximum(x, 0), 1)


def sphere_box(P, r, hb):
    """Sphere (centre P (..., 3) in the box frame, radius r) against the solid cube of half edge hb: signed distance, local
    normal, witness on the cube, `inside` (the centre-inside rule was used) and the margin of the face choice."""
    q = np.clip(P, -hb, hb)
    d = P - q
    d2 = _dot(d, d)
    out = d2 > 1e-12
    dist = np.sqrt(np.where(out, d2, 1))
    n_out = d / dist[..., None]
    pen = hb - np.abs(P)
    ax = np.argmin(pen, -1)                                       # the first axis wins a tie
    onehot = np.arange(3) == ax[..., None]
    sgn = np.where(np.take_along_axis(P, ax[..., None], -1)[..., 0] >= 0, 1, -1).astype(P.dtype)
    n_in = onehot * sgn[..., None]
    p_in = np.where(onehot, sgn[..., None] * hb, P)
    best = np.take_along_axis(pen, ax[..., None], -1)[..., 0]
    gap = np.where(out, dist - r, -best - r)
    ps = np.sort(pen, -1)
    return (gap.astype(P.dtype), np.where(out[..., None], n_out, n_in).astype(P.dtype), np.where(out[..., None], q, p_in).astype(P.dtype),
            ~out, ps[..., 1] - ps[..., 0])


def seg_box(a, e, r, hb):
    """Capsule axis P(t) = a + t e ((..., 3), box frame), radius r, against the cube of half edge hb.  Returns a dict: d, n, p (box
    frame), t, axis_dist (distance of the axis to the cube at the minimiser), meets, unique (the minimiser of f is unique, judged
    at the working precision: meaningful in float64), face_margin (inside rule: runner-up depth minus depth)."""
    T = a.dtype.type
    hb = T(hb)
    mv = np.abs(e) > 0
    es = np.where(mv, e, 1)
    t1, t2 = np.where(mv, (-hb - a) / es, 0), np.where(mv, (hb - a) / es, 0)
    shape = a.shape[:-1] + (1,)
    cand = np.sort(np.concatenate([np.zeros(shape, a.dtype), np.ones(shape, a.dtype), _clip01(t1), _clip01(t2)], -1), -1)   # (..., 8)

    def g_of(t):                                                  # f'(t) / 2
        P = a[..., None, :] + t[..., None] * e[..., None, :]
        return _dot(P - np.clip(P, -hb, hb), e[..., None, :])

    g = g_of(cand)
    pos = g >= 0
    k = np.argmax(pos, -1)                                         # the first candidate where f' >= 0
    none = ~pos.any(-1)
    km = np.maximum(k - 1, 0)
    pick = lambda x, i: np.take_along_axis(x, i[..., None], -1)[..., 0]
    tl, th, gl, gh = pick(cand, km), pick(cand, k), pick(g, km), pick(g, k)
    den = gh - gl
    troot = tl + (th - tl) * (-gl / np.where(den > 0, den, 1))
    ts = np.where(none, 1, np.where(k == 0, 0, np.minimum(np.maximum(troot, tl), th))).astype(a.dtype)
    Ps = a + ts[..., None] * e
    ex = Ps - np.clip(Ps, -hb, hb)
    axis_dist = np.sqrt(_dot(ex, ex))
    meets = ~(_dot(ex, ex) > T(MEET * MEET))
    # the stretch of the axis inside the cube, by slab clipping
    outside = np.abs(a) > hb
    lo = np.where(mv, np.minimum(t1, t2), np.where(outside, 2, 0))
    hi = np.where(mv, np.maximum(t1, t2), np.where(outside, -1, 1))
    tin, tout = np.maximum(lo.max(-1), 0), np.minimum(hi.min(-1), 1)
    tw = np.where(meets & (tin <= tout), T(0.5) * (tin + tout), ts).astype(a.dtype)
    d, n, p, inside, margin = sphere_box(a + tw[..., None] * e, r, hb)
    after = cand > (ts[..., None] + T(1e-12))
    g_next = np.where(after, g, np.inf).min(-1)
    unique = ~meets & (g_next > 1e-9 * np.sqrt(_dot(e, e)) * np.maximum(axis_dist, 1e-30))
    return dict(d=d, n=n, p=p, t=tw, axis_dist=axis_dist.astype(a.dtype), meets=meets, inside=inside, unique=unique, face_margin=margin)


def seg_seg(p1, d1, p2, d2):
    """Clamped closest points p1 + s d1, p2 + t d2 of two segments ((..., 3) arrays), the header's two-stage clamping.  Returns
    s, t, the difference c_A - c_B, its length and sin^2 of the angle between the axes (1 for a zero-length axis)."""
    r = p1 - p2
    a, e, b, c, f = _dot(d1, d1), _dot(d2, d2), _dot(d1, d2), _dot(d1, r), _dot(d2, r)
    za, ze = ~(a > ZERO_AXIS2), ~(e > ZERO_AXIS2)
    ae = a * e
    den = ae - b * b
    par = za | ze | ~(den > PARALLEL * ae)
    s1 = np.where(par, 0, _clip01((b * f - c * e) / np.where(par, 1, den)))
    traw = np.where(ze, 0, (b * s1 + f) / np.where(ze, 1, e))
    t = _clip01(traw)
    s2 = np.where(za, 0, _clip01((b * t - c) / np.where(za, 1, a)))
    s = np.where(ze | (traw != t), s2, s1)
    diff = (p1 + s[..., None] * d1) - (p2 + t[..., None] * d2)
    sin2 = np.where(za | ze, 1, den / np.where(za | ze, 1, ae))
    return s.astype(p1.dtype), t.astype(p1.dtype), diff.astype(p1.dtype), np.sqrt(_dot(diff, diff)).astype(p1.dtype), sin2


class HandProx:
    """The clearance queries of the header for rows of joint positions and box poses."""

    def __init__(self, model_struct, sim_cfg):
        self.geom = HandGeometry(model_struct)
        self.r = self.geom.cap_r.copy()
        self.box_size = float(sim_cfg.box_size)
        self.pairs = np.array(pair_table())

    def test_poses(self, n, seed):
        """n rows (q (n, 26), box_pose (n, 7)) as float32: joints uniform in their limits, base slides +-0.3 m, base rotations
        +-1 rad; box centre = palm joint origin + U(-0.12, 0.12)^3, random orientation."""
        rng = np.random.default_rng(seed)
        q = rng.uniform(self.geom.lo, self.geom.hi, size=(n, _abi.NJ))
        q[:, :3] = rng.uniform(-0.3, 0.3, size=(n, 3))
        q[:, 3:6] = rng.uniform(-1.0, 1.0, size=(n, 3))
        q = q.astype(np.float32)
        quat = rng.normal(size=(n, 4))
        quat /= np.linalg.norm(quat, axis=1, keepdims=True)
        off = rng.uniform(-0.12, 0.12, size=(n, 3))
        o5 = np.stack([self.geom.fk(q[i].astype(np.float64))[0][5] for i in range(n)])
        return q, np.concatenate([o5 + off, quat], 1).astype(np.float32)

    def capsules(self, q, dtype=np.float64):
        """World axis ends a, b (n, 18, 3) and the palm joint origins (n, 3) for joint positions q (n, 26)."""
        dt = np.dtype(dtype)
        a, b, o5 = [], [], []
        for row in np.asarray(q):
            ai, bi, (o, _) = self.geom.capsules(row.astype(dt), dtype)
            a.append(ai), b.append(bi), o5.append(o[5])
        return np.stack(a).astype(dt), np.stack(b).astype(dt), np.stack(o5).astype(dt)

    def ground(self, a, b):
        """(n, 18, 8) ground records and |z0 - z1| (the margin of the choice of the lower end)."""
        r = self.r.astype(a.dtype)
        up = b[..., 2] < a[..., 2]
        el = np.where(up[..., None], b, a)
        rec = np.zeros(a.shape[:-1] + (8,), a.dtype)
        rec[..., 0] = el[..., 2] - r
        rec[..., 3] = 1
        rec[..., 4:6] = el[..., :2]
        rec[..., 7] = up
        return rec, np.abs(a[..., 2] - b[..., 2])

    def box(self, a, b, box_pose, size=None):
        """(n, 18, 8) box records and the dict of seg_box (axis_dist, meets, unique, face_margin) for box poses (n, 7)."""
        dt = a.dtype
        hb = 0.5 * (self.box_size if size is None else float(size))
        R = np.stack([quat_to_mat(p[3:7], dt.type) for p in np.asarray(box_pose, dtype=np.float64)])   # (n, 3, 3) world <- box
        c = np.asarray(box_pose)[:, None, :3].astype(dt)
        al = np.einsum("nji,ncj->nci", R, a - c)
        el = np.einsum("nji,ncj->nci", R, b - a)
        out = seg_box(al, el, self.r.astype(dt)[None, :], hb)
        rec = np.zeros(a.shape[:-1] + (8,), dt)
        rec[..., 0] = out["d"]
        rec[..., 1:4] = np.einsum("nij,ncj->nci", R, out["n"])
        rec[..., 4:7] = np.einsum("nij,ncj->nci", R, out["p"]) + c
        rec[..., 7] = out["t"]
        return rec, out

    def pair_records(self, a, b):
        """All 120 pairs: dict d (n, 120), n (n, 120, 3), p = witness on B's surface (n, 120, 3), sin2 (n, 120)."""
        dt = a.dtype
        ia, ib = self.pairs[:, 0], self.pairs[:, 1]
        ra, rb = self.r.astype(dt)[ia], self.r.astype(dt)[ib]
        s, t, diff, ln, sin2 = seg_seg(a[:, ia], b[:, ia] - a[:, ia], a[:, ib], b[:, ib] - a[:, ib])
        far = ln >= 1e-9
        n = np.where(far[..., None], diff / np.where(far, ln, 1)[..., None], np.array([0, 0, 1], dt))
        cb = a[:, ib] + t[..., None] * (b[:, ib] - a[:, ib])
        return dict(d=(ln - ra - rb).astype(dt), n=n.astype(dt), p=(cb + rb[:, None] * n).astype(dt), sin2=sin2)

    def self_min(self, pr):
        """(n, 15, 8) records of the closest pair per group (word 7: the pair index as a number), the pair indices (n, 15) and how
        far the runner-up of each group is behind."""
        n = pr["d"].shape[0]
        rec = np.zeros((n, NGROUP, 8), pr["d"].dtype)
        idx = np.zeros((n, NGROUP), np.int64)
        margin = np.zeros((n, NGROUP))
        rows = np.arange(n)
        for g in range(NGROUP):
            members = np.nonzero(self.pairs[:, 2] == g)[0]
            d = pr["d"][:, members]
            k = np.argmin(d, 1)                                    # the lowest index wins a tie
            i = members[k]
            rec[:, g, 0], rec[:, g, 1:4], rec[:, g, 4:7], rec[:, g, 7] = pr["d"][rows, i], pr["n"][rows, i], pr["p"][rows, i], i
            idx[:, g] = i
            ds = np.sort(d.astype(np.float64), 1)
            margin[:, g] = ds[:, 1] - ds[:, 0]
        return rec, idx, margin

    def query(self, q, box_pose=None, size=None, dtype=np.float64):
        """Everything the device call returns, at `dtype`, plus the conditioning data of the records."""
        a, b, _ = self.capsules(q, dtype)
        gr, gmargin = self.ground(a, b)
        cap_env = np.zeros(a.shape[:-1] + (2, 8), a.dtype)
        cap_env[:, :, 1] = gr
        aux = None
        if box_pose is None:
            cap_env[:, :, 0, 0] = np.inf
        else:
            cap_env[:, :, 0], aux = self.box(a, b, box_pose, size)
        pr = self.pair_records(a, b)
        sm, idx, margin = self.self_min(pr)
        return dict(cap_env=cap_env, self_min=sm, pair_dist=pr["d"], pair=pr, min_idx=idx, min_margin=margin, box=aux,
                    ground_margin=gmargin, a=a, b=b)


# ------------------------------------------------------------------------------------------------- what the suites that query share
ROWS, SEED = 70, 23                                        # the rows of tests/test_proximity.py
SHAPES = {"cap_env": (NCAP, 2, 8), "self_min": (NGROUP, 8), "pair_dist": (NPAIR,)}
ALL = ("cap_env", "self_min", "pair_dist")


def select(r64):
    """The well-conditioned records of a float64 reference result (docstring of tests/test_proximity.py)."""
    rows = np.arange(r64["min_idx"].shape[0])[:, None]
    sel = dict(group=(r64["min_margin"] > 1e-4) & (r64["pair"]["sin2"][rows, r64["min_idx"]] >= 0.0025),
               pair=r64["pair"]["sin2"] >= 0.0025, ground=r64["ground_margin"] > 1e-5)
    if r64["box"] is not None:
        bx = r64["box"]
        zone = (bx["axis_dist"] > 1e-7) & (bx["axis_dist"] < 1e-5)
        sel["box_d"] = ~zone
        sel["box"] = (bx["unique"] & (bx["axis_dist"] >= 1e-5)) | (bx["meets"] & ~zone & (bx["face_margin"] > 1e-4))
    return sel


def reference(hp, q, box, size=None):
    """float64 and float32 reference of the rows, the selections and the tolerances: 4 x the float32-vs-float64 difference."""
    r64, r32 = hp.query(q, box, size), hp.query(q, box, size, dtype=np.float32)
    assert r32["cap_env"].dtype == np.float32 and r32["pair_dist"].dtype == np.float32
    sel = select(r64)
    diff = lambda a, b, m=None: float(np.abs(a.astype(np.float64) - b)[... if m is None else m].max())
    e = dict(ground_d=diff(r32["cap_env"][:, :, 1, 0], r64["cap_env"][:, :, 1, 0]),
             ground_p=diff(r32["cap_env"][:, :, 1, 4:7], r64["cap_env"][:, :, 1, 4:7], sel["ground"]),
             pair_d=diff(r32["pair_dist"], r64["pair_dist"]),
             group_n=diff(r32["self_min"][..., 1:4], r64["self_min"][..., 1:4], sel["group"]),
             group_p=diff(r32["self_min"][..., 4:7], r64["self_min"][..., 4:7], sel["group"]))
    assert (r32["min_idx"][sel["group"]] == r64["min_idx"][sel["group"]]).all()
    if box is not None:
        b32, b64 = r32["cap_env"][:, :, 0], r64["cap_env"][:, :, 0]
        e.update(box_d=diff(b32[..., 0], b64[..., 0], sel["box_d"]), box_n=diff(b32[..., 1:4], b64[..., 1:4], sel["box"]),
                 box_p=diff(b32[..., 4:7], b64[..., 4:7], sel["box"]), box_t=diff(b32[..., 7], b64[..., 7], sel["box"]))
    return dict(r64=r64, sel=sel, e=e, tol={k: 4 * v for k, v in e.items()})


def gpu_query(core, k, env_ids=None, q=None, box=None, size=0.0, want=ALL):
    """core.proximity into guarded outputs: dict of numpy arrays by output name."""
    import torch
    bufs = {o: guarded(k, *SHAPES[o]) for o in want}
    dev = lambda x: None if x is None else torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device=core.device)
    core.proximity(env_ids=env_ids, q=dev(q), box_pose=dev(box), box_size=size, **{o: v for o, (_, v) in bufs.items()})
    for full, _ in bufs.values():
        guards_ok(full)
    return {o: v.cpu().numpy() for o, (_, v) in bufs.items()}


def _err(dev, ref, mask=None):
    d = np.abs(dev.astype(np.float64) - ref)
    return float(d[... if mask is None else mask].max())


def check_against(out, ref, box=True, label=""):
    """The distance and well-conditioned-record checks of tests/test_proximity.py's docstring; returns the measured device errors."""
    r64, sel, tol = ref["r64"], ref["sel"], ref["tol"]
    assert not any(np.isnan(v).any() for v in out.values()), "an element was not written"
    m = {}
    ce, sm = out["cap_env"], out["self_min"]
    m["ground_d"] = _err(ce[:, :, 1, 0], r64["cap_env"][:, :, 1, 0])
    m["ground_p"] = _err(ce[:, :, 1, 4:7], r64["cap_env"][:, :, 1, 4:7], sel["ground"])
    m["pair_d"] = _err(out["pair_dist"], r64["pair_dist"])
    m["group_d"] = _err(sm[..., 0], r64["self_min"][..., 0])
    m["group_n"] = _err(sm[..., 1:4], r64["self_min"][..., 1:4], sel["group"])
    m["group_p"] = _err(sm[..., 4:7], r64["self_min"][..., 4:7], sel["group"])
    if box:
        b, b64 = ce[:, :, 0], r64["cap_env"][:, :, 0]
        m["box_d"] = _err(b[..., 0], b64[..., 0], sel["box_d"])
        m["box_n"], m["box_p"] = _err(b[..., 1:4], b64[..., 1:4], sel["box"]), _err(b[..., 4:7], b64[..., 4:7], sel["box"])
        m["box_t"] = _err(b[..., 7], b64[..., 7], sel["box"])
    print(f"{label}device against the float64 reference:", {k: f"{v:.3g}" for k, v in m.items()})
    print(f"{label}bounds (4 x reference float32 against float64):", {k: f"{v:.3g}" for k, v in tol.items()})
    # exact parts of the contract
    assert (ce[:, :, 1, 1:4] == np.array([0, 0, 1], np.float32)).all() and (ce[:, :, 1, 6] == 0).all()
    assert (ce[:, :, 1, 7][sel["ground"]] == r64["cap_env"][:, :, 1, 7][sel["ground"]]).all() and np.isin(ce[:, :, 1, 7], (0, 1)).all()
    idx = bits(sm[..., 7])
    assert (idx[sel["group"]] == r64["min_idx"][sel["group"]]).all(), "a group's closest pair differs on a well-conditioned record"
    rows = np.arange(idx.shape[0])[:, None]
    assert (hp_pairs_group(idx) == np.arange(NGROUP)[None, :]).all()                # every record names a pair of its own group ...
    assert (bits(sm[..., 0]) == bits(out["pair_dist"][rows, idx])).all()       # ... and carries that pair's distance, bit for bit
    for g in range(NGROUP):                                                        # the minimum of the group, ties to the lowest index
        members = np.nonzero(PAIR_GROUP == g)[0]
        d = out["pair_dist"][:, members]
        assert (members[np.argmin(d, 1)] == idx[:, g]).all()
    for k in ("ground_d", "ground_p", "pair_d", "group_n", "group_p") + (("box_d", "box_n", "box_p", "box_t") if box else ()):
        assert m[k] <= tol[k], (k, m[k], tol[k])
    assert m["group_d"] <= tol["pair_d"], ("group_d", m["group_d"], tol["pair_d"])
    return m


PAIR_GROUP = np.array([t[2] for t in pair_table()])


def hp_pairs_group(idx):
    assert ((idx >= 0) & (idx < NPAIR)).all()
    return PAIR_GROUP[idx]
