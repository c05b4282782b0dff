"""Clearance queries on the device (dexsim_query_proximity, env.query_proximity) against tests/proximity_ref.py, a numpy statement of
the geometry include/dexsim.h specifies, run in float64 and, for the roundoff figures, in float32.

Test poses (proximity_ref.HandProx.test_poses, 70 rows from a fixed seed): joints uniform in their limits, base slides +-0.3 m, base
rotations +-1 rad; box centre = palm joint origin + U(-0.12, 0.12)^3 with a random orientation; everything rounded to float32
before either side sees it.

Tolerances (test_against_reference prints every figure before it asserts):
  * distances -- all 70 x (36 + 15 + 120): 4 x the largest difference between the reference's own float32 and float64 values of
    that kind of record (ground, box, pairs) on the same 70 rows, recomputed by the test.  The factor 4 is the project's standing
    allowance for a different order of the same fp32 arithmetic plus sincos_joint (tests/test_kindyn.py, tests/test_ik.py).  An
    index, sign, radius or pairing bug is at least a capsule radius (6.5 mm).  Left out: box records whose float64 axis distance
    is in (1e-7, 1e-5) m, the boundary between the outside and the inside rule (1e-6 m), where roundoff may pick the other rule.
  * normals, witness points, t, the group's pair index -- on the well-conditioned records only: groups whose runner-up is more
    than 1e-4 m behind and whose closest pair has sin^2 of the axis angle >= 0.0025; box records whose float64 minimiser is unique,
    and records of the inside rule whose face choice is more than 1e-4 m ahead of the runner-up (the face is an argmin like the
    group's pair); ground records whose two ends differ by more than 1e-5 m in height.  The bound is 4 x the reference's
    float32-vs-float64 difference of that quantity on those records; pair indices must be equal.  At least 90 % of the records of
    each kind must be selected.
Every GPU test uses N = 70: two workgroups, six live lanes in the second.  Every device output sits between two guard rows that must
come back untouched.

Measured on one MI355X (profiles/proximity/README.md has the full list): distances off the float64 reference by 9.6e-8 m (ground,
bound 4.3e-7), 1.3e-7 m (box, bound 3.4e-7), 5.2e-8 m (pairs, bound 4.2e-7); 98.9 % of the groups and all box records selected.
"""
import ctypes as C

import numpy as np
import pytest

from dexrobot_isaac_amd import _abi
from tests import proximity_ref as pr
from tests.query_rig import (bits, guarded as _guarded, guards_ok as _guards_ok, load_lib, pose_core, same as _same, setup as _setup,
                             snapshot as _snapshot, stub_core)

N, SEED = pr.ROWS, pr.SEED
NJ, NCAP, NG, NP = _abi.NJ, _abi.NCAP, _abi.NPROX_GROUPS, _abi.NPROX_PAIRS
SHAPES, ALL = pr.SHAPES, pr.ALL
_reference, gpu_query, _check_against = pr.reference, pr.gpu_query, pr.check_against


# ------------------------------------------------------------------------------------------------- CPU
@pytest.fixture(scope="module")
def lib():
    return load_lib()


def test_abi_exports_pair_table_and_argument_errors(lib):
    for name in ("dexsim_proximity_pair", "dexsim_query_proximity"):
        assert name in _abi.EXPORTED_SYMBOLS
        assert hasattr(lib, name), f"libdexsim.so does not export {name}"
    a, b, g = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    table = []
    for i in range(NP):
        assert lib.dexsim_proximity_pair(i, C.byref(a), C.byref(b), C.byref(g)) == 0
        table.append((a.value, b.value, g.value))
    assert table == pr.pair_table()
    assert [t[2] for t in table] == sorted(t[2] for t in table) and len(set(table)) == NP
    for i in (-1, NP):
        assert lib.dexsim_proximity_pair(i, C.byref(a), C.byref(b), C.byref(g)) == 1 and b"out of range" in lib.dexsim_last_error()
    assert lib.dexsim_proximity_pair(0, None, C.byref(b), C.byref(g)) == 1 and b"null" in lib.dexsim_last_error()

    buf = (C.c_float * 64)()
    base = C.addressof(buf)
    base += (-base) % 16
    p, odd = C.c_void_p(base), C.c_void_p(base + 4)                            # never written: every call below fails before a launch

    def call(h=None, k=1, size=0.0, cap_env=p, self_min=p, pair_dist=p):
        rc = lib.dexsim_query_proximity(h, None, k, None, None, size, cap_env, self_min, pair_dist, None)
        return rc, lib.dexsim_last_error()

    cases = [
        (dict(), b"null handle"),
        (dict(k=0), b"k must be positive"), (dict(k=-3), b"k must be positive"),
        (dict(cap_env=None, self_min=None, pair_dist=None), b"at least one"),
        (dict(cap_env=odd), b"16-byte aligned"), (dict(self_min=odd), b"16-byte aligned"), (dict(pair_dist=odd), b"16-byte aligned"),
        (dict(cap_env=None, self_min=None, pair_dist=odd), b"16-byte aligned"),
        (dict(size=float("nan")), b"box_size"), (dict(size=float("inf")), b"box_size"), (dict(size=-float("inf")), b"box_size"),
    ]
    for kw, text in cases:
        rc, msg = call(**kw)
        assert rc == 1 and text in msg, (kw, rc, msg)                          # DEXSIM_ERR_ARG with its text
    assert not any(buf)
    assert (_abi.NPROX_GROUPS, _abi.NPROX_PAIRS) == (15, 120)


def _point_box_dist(P, hb):
    d = P - np.clip(P, -hb, hb)
    return np.sqrt((d * d).sum(-1))


def _brute_cases(rng, n):
    """Segment / cube cases in the cube's frame (half edge hb): general position, axes parallel to a face, minima at an end, axes
    through the cube."""
    hb = 0.03
    a = rng.uniform(-0.12, 0.12, size=(n, 3))
    e = rng.uniform(-0.08, 0.08, size=(n, 3))
    kind = np.arange(n) % 4
    par = kind == 1                                                            # parallel to one or two faces: exact zeros in the axis
    e[par, 0] = 0.0
    e[par & (np.arange(n) % 8 == 5), 1] = 0.0
    end = kind == 2                                                            # pointing away from the cube: the minimum is at t = 0
    a[end] = np.sign(a[end]) * (hb + np.abs(a[end]))
    e[end] = np.sign(a[end]) * np.abs(e[end])
    thru = kind == 3                                                           # through the cube
    mid = rng.uniform(-0.8 * hb, 0.8 * hb, size=(n, 3))
    a[thru] = (mid - 0.5 * e)[thru]
    e[thru & (np.arange(n) % 8 == 7), 2] = 0.0                                  # ... some of them parallel to a face as well
    return a, e, hb


def test_reference_against_brute_force():
    rng = np.random.default_rng(5)
    n, S = 2000, 4001
    ts = np.linspace(0.0, 1.0, S)
    # segment / cube
    a, e, hb = _brute_cases(rng, n)
    r = rng.uniform(0.005, 0.0125, size=n)
    out = pr.seg_box(a, e, r, hb)
    worst_hi, worst_lo = 0.0, 0.0
    for lo in range(0, n, 250):
        sl = slice(lo, lo + 250)
        P = a[sl, None, :] + ts[None, :, None] * e[sl, None, :]
        brute = _point_box_dist(P, hb).min(1)
        lip = np.linalg.norm(e[sl], axis=1) / (S - 1)
        ref = out["axis_dist"][sl]
        worst_hi, worst_lo = max(worst_hi, float((ref - brute).max())), max(worst_lo, float((brute - lip - ref).max()))
        assert (ref <= brute + 1e-15).all()                                    # the reference is the minimum ...
        assert (ref >= brute - lip - 1e-15).all()                              # ... and no sample can be further below it than the spacing allows
    m = out["meets"]
    assert m.sum() >= 300 and (~m).sum() >= 1200
    assert (out["d"][m] <= -r[m]).all() and (out["d"][~m] > -r[~m]).all()
    on_face = np.isclose(np.abs(out["p"]), hb, rtol=0, atol=1e-15).any(-1) & (np.abs(out["p"]) <= hb + 1e-15).all(-1)
    assert on_face[m].all()                                                    # axis meets the cube: the witness lies on a face
    assert (out["t"] >= 0).all() and (out["t"] <= 1).all()
    # outside: d + r is the axis distance, the witness is the clamped axis point, n the unit excess
    Pw = a + out["t"][:, None] * e
    o = ~m
    assert np.abs(out["d"][o] + r[o] - out["axis_dist"][o]).max() <= 1e-15
    assert np.abs(out["p"][o] + (out["d"][o] + r[o])[:, None] * out["n"][o] - Pw[o]).max() <= 1e-15
    # the smallest t on a flat stretch: an axis parallel to a face above it, crossing the face's shadow
    flat = pr.seg_box(np.array([[-0.1, 0.0, 0.05]]), np.array([[0.2, 0.0, 0.0]]), np.array([0.01]), hb)
    assert abs(flat["t"][0] - 0.35) <= 1e-15 and abs(flat["d"][0] - 0.01) <= 1e-15 and not flat["unique"][0]
    print(f"segment / cube: reference above the sampled minimum by at most {worst_hi:.3g}, below it (beyond the Lipschitz bound) by {worst_lo:.3g}")

    # segment / segment
    p1, p2 = rng.uniform(-0.1, 0.1, size=(n, 3)), rng.uniform(-0.1, 0.1, size=(n, 3))
    d1, d2 = rng.uniform(-0.08, 0.08, size=(n, 3)), rng.uniform(-0.08, 0.08, size=(n, 3))
    kind = np.arange(n) % 5
    d2[kind == 1] = d1[kind == 1] * rng.uniform(-1.5, 1.5, size=(n, 1))[kind == 1]   # parallel axes
    d1[kind == 2] = 0.0                                                        # A is a point
    d2[kind == 3] = 0.0                                                        # B is a point
    both = (kind == 3) & (np.arange(n) % 10 == 8)
    d1[both] = 0.0
    s, t, diff, ln, sin2 = pr.seg_seg(p1, d1, p2, d2)
    assert (s >= 0).all() and (s <= 1).all() and (t >= 0).all() and (t <= 1).all() and np.isfinite(ln).all()
    for lo in range(0, n, 250):
        sl = slice(lo, lo + 250)
        X = p1[sl, None, :] + ts[None, :, None] * d1[sl, None, :]              # samples of A; B by the exact point / segment distance
        ee = (d2[sl] * d2[sl]).sum(-1)
        tt = np.clip(((X - p2[sl, None, :]) * d2[sl, None, :]).sum(-1) / np.where(ee > 0, ee, 1)[:, None], 0, 1) * (ee > 0)[:, None]
        brute = np.linalg.norm(X - (p2[sl, None, :] + tt[..., None] * d2[sl, None, :]), axis=-1).min(1)
        lip = np.linalg.norm(d1[sl], axis=1) / (S - 1)
        assert (ln[sl] <= brute + 1e-15).all() and (ln[sl] >= brute - lip - 1e-15).all()


_stub_core = stub_core(dict(proximity=lambda **kw: kw), proximity_pairs=lambda self: pr.pair_table())


def test_env_argument_validation():
    import torch
    from dexrobot_isaac_amd import make_env
    from oracle.py_backend import OracleCore
    env = make_env("BlindGrasping", 3, "cpu", "cpu", 0, _core_factory=_stub_core)
    q3 = torch.zeros(3, NJ)
    bad = [
        (dict(q=torch.zeros(3, NJ - 1)), "q must have shape"), (dict(env_ids=[]), "empty"),
        (dict(outputs=()), "outputs"), (dict(outputs=("cap_env", "contacts")), "outputs"),
        (dict(box_pose="world"), "box_pose"), (dict(box_pose="env"), "box_pose='env'"), (dict(box_pose="env", q=torch.zeros(2, NJ)), "box_pose='env'"),
        (dict(box_pose=torch.zeros(3, 6)), "box_pose must have shape"), (dict(box_pose=torch.zeros(2, 7), q=q3), "box_pose must have shape"),
        (dict(box_size=0.0), "box_size"), (dict(box_size=-0.05), "box_size"), (dict(box_size=float("nan")), "box_size"),
        (dict(box_size=float("inf")), "box_size"),
        (dict(out=[torch.zeros(3, NP)]), "out must be a dict"), (dict(out={"pair_dist": torch.zeros(3, NP)}, outputs=("self_min",)), "out must be a dict"),
        (dict(out={"pair_dist": torch.zeros(2, NP)}), "out must be a contiguous float32 tensor"),
        (dict(out={"pair_dist": torch.zeros(3, NP, dtype=torch.float64)}), "out must be a contiguous float32 tensor"),
    ]
    for kw, text in bad:
        with pytest.raises(ValueError, match=text):
            env.query_proximity(**kw)
    assert not env._core.calls                                                 # nothing reached the core
    res = env.query_proximity()
    kw = env._core.calls[-1]
    assert kw["env_ids"] is None and kw["q"] is None and kw["box_pose"] is None and kw["box_size"] == 0.0
    assert res.cap_env.shape == (3, NCAP, 2, 8) and res.self_min.shape == (3, NG, 8) and res.pair_dist.shape == (3, NP)
    assert res.pairs.shape == (NP, 3) and res.pairs.tolist() == [list(t) for t in pr.pair_table()]
    assert res.capsule_body(0) == res.capsule_body(2) == env.model.body_names[6]
    assert res.capsule_body(3 + 3 * 1 + 2) == "r_f_link2_4" and res.group_fingers(0) == ("thumb", "index")
    assert res.group_fingers(9) == ("ring", "pinky") and res.group_fingers(12) == ("palm", "middle")
    mine = torch.zeros(2, NP)
    res = env.query_proximity(env_ids=[2, 0], outputs="pair_dist", out={"pair_dist": mine}, box_size=0.07)
    kw = env._core.calls[-1]
    assert res.pair_dist is mine and res.cap_env is None and res.self_min is None and set(kw) >= {"pair_dist"} and "cap_env" not in kw
    assert kw["env_ids"].tolist() == [2, 0] and abs(kw["box_size"] - 0.07) < 1e-12
    res = env.query_proximity(q=q3, box_pose="env", outputs=("cap_env",))      # "check my IK result against my box"
    kw = env._core.calls[-1]
    assert kw["box_pose"].shape == (3, 7) and torch.equal(kw["box_pose"], env._core.root_state[:, 1, :7]) and kw["q"].shape == (3, NJ)
    res = env.query_proximity(q=torch.zeros(5, NJ), box_pose=torch.zeros(5, 7))
    assert res.pair_dist.shape == (5, NP) and env._core.calls[-1]["box_pose"].shape == (5, 7)
    nobox = make_env("BaseTask", 3, "cpu", "cpu", 0, _core_factory=_stub_core)
    with pytest.raises(ValueError, match="needs a task with a box"):
        nobox.query_proximity(q=q3, box_pose="env")
    plain = make_env("BaseTask", 2, "cpu", "cpu", 0, _core_factory=OracleCore)  # the CPU stand-in has no clearance query
    with pytest.raises(NotImplementedError):
        plain.query_proximity()


# ------------------------------------------------------------------------------------------------- the reference on the test poses
@pytest.fixture(scope="module")
def hp():
    sc, ms = _setup(N)
    return pr.HandProx(ms, sc)


@pytest.fixture(scope="module")
def poses(hp):
    q, box = hp.test_poses(N, SEED)
    ref = _reference(hp, q, box)
    return dict(q=q, box=box, **ref)


@pytest.fixture(scope="module")
def hp_generic():
    """The reference on the model of tests/generic_model.py: every capsule starts off its joint origin and ends off the x axis."""
    sc, ms = _setup(N, model="generic")
    return pr.HandProx(ms, sc)


@pytest.fixture(scope="module")
def poses_generic(hp_generic):
    q, box = hp_generic.test_poses(N, SEED)
    return dict(q=q, box=box, **_reference(hp_generic, q, box))


def test_reference_roundoff_and_selection_generic_model(hp_generic, poses_generic):
    test_reference_roundoff_and_selection(hp_generic, poses_generic)


def test_reference_roundoff_and_selection(hp, poses):
    """The measurement the GPU bars rest on: the reference's own float32-vs-float64 differences on the 70 rows, and how many
    records are well-conditioned."""
    e, sel = poses["e"], poses["sel"]
    frac = {k: float(v.mean()) for k, v in sel.items()}
    print("reference float32 against float64:", {k: f"{v:.3g}" for k, v in e.items()})
    print("selected:", {k: f"{v:.4f}" for k, v in frac.items()}, "axis meets the box:", f"{poses['r64']['box']['meets'].mean():.4f}")
    assert all(0 < e[k] < 2e-6 for k in ("ground_d", "pair_d", "box_d"))        # roundoff of metres-sized fp32 numbers, not a branch flip
    assert all(frac[k] >= 0.9 for k in ("group", "pair", "box", "ground")) and frac["box_d"] >= 0.99


# ------------------------------------------------------------------------------------------------- GPU helpers
@pytest.fixture(scope="module")
def rig(hp, poses):
    """A BlindGrasping core of N envs posed at the test poses (hand and box), and its full query, computed once."""
    from dexrobot_isaac_amd.core import DexSimCore
    sc, ms = _setup(N)
    core = DexSimCore(sc, ms, "cuda:0")
    core.reset()
    pose_core(core, poses["q"], poses["box"])
    return dict(core=core, full=gpu_query(core, N))


# ------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_against_reference(rig, hp, poses):
    """Measured on one MI355X: see profiles/proximity/README.md."""
    out, r64, sel = rig["full"], poses["r64"], poses["sel"]
    for k, v in sel.items():
        print(f"selected {k}: {v.mean():.4f}")
        assert v.mean() >= 0.9
    m = _check_against(out, poses)
    # the record's own identities, against the float64 axes: axis point = p + (d + r) n, |n| = 1
    a, b, r = r64["a"], r64["b"], hp.r
    box = out["cap_env"][:, :, 0].astype(np.float64)
    ok = sel["box"] & ~r64["box"]["meets"]
    axis_pt = a + box[..., 7:8] * (b - a)
    ident = float(np.abs(box[..., 4:7] + (box[..., 0:1] + r[None, :, None]) * box[..., 1:4] - axis_pt)[ok].max())
    print(f"box records: |p + (d + r) n - axis point| <= {ident:.3g}")
    assert ident <= poses["tol"]["box_p"] + poses["tol"]["box_d"]
    assert np.abs(np.linalg.norm(box[..., 1:4], axis=-1) - 1).max() <= 1e-6
    assert np.abs(np.linalg.norm(out["self_min"][..., 1:4].astype(np.float64), axis=-1) - 1).max() <= 1e-6
    inside = r64["box"]["meets"] & sel["box_d"]
    assert (out["cap_env"][:, :, 0, 0][inside] <= -r[None, :].repeat(N, 0)[inside].astype(np.float32)).all()
    assert m["box_d"] < 6.5e-3 and m["pair_d"] < 6.5e-3


@pytest.mark.gpu
def test_structure_free_model(hp_generic, poses_generic):
    """test_against_reference on the model of tests/generic_model.py, the bounds recomputed on its rows."""
    from dexrobot_isaac_amd.core import DexSimCore
    sc, ms = _setup(N, model="generic")
    core = DexSimCore(sc, ms, "cuda:0")
    core.reset()
    pose_core(core, poses_generic["q"], poses_generic["box"])
    test_against_reference(dict(core=core, full=gpu_query(core, N)), hp_generic, poses_generic)
    core.close()


@pytest.mark.gpu
def test_row_contract():
    import torch
    from dexrobot_isaac_amd import make_env
    env = make_env("BlindGrasping", N, "cuda:0", "cuda:0", 0)
    env.reset()
    g = torch.Generator().manual_seed(9)
    for _ in range(10):
        env.step((2 * torch.rand(N, env.num_actions, generator=g) - 1).cuda())
    core = env._core
    before, state0 = _snapshot(core), env.get_state()
    full = gpu_query(core, N)
    assert not any(np.isnan(v).any() for v in full.values())
    assert np.isfinite(full["cap_env"]).all()                                  # the env has a box
    # the override path fed the published state gives the state path's bits
    q = core.dof_state[:, :, 0].cpu().numpy()
    box = core.root_state[:, 1, :7].cpu().numpy()
    over = gpu_query(core, N, q=q, box=box, env_ids=[-1])                      # env_ids is ignored with an override
    for k in ALL:
        assert (bits(over[k]) == bits(full[k])).all(), k
    # the same through the public surface, with the env's own box gathered by name
    res = env.query_proximity(q=env.dof_pos.clone(), box_pose="env")
    torch.cuda.synchronize()
    for k in ALL:
        assert (bits(getattr(res, k).cpu().numpy()) == bits(full[k])).all(), k
    assert (res.min_pair.cpu().numpy() == bits(full["self_min"][..., 7])).all()
    # a permuted id list with one id out of range
    ids = [69, 0, 64, N, 3, 63, -1, 37]
    good = [i for i, e in enumerate(ids) if 0 <= e < N]
    by_id = gpu_query(core, len(ids), env_ids=ids)
    for k in ALL:
        assert (bits(by_id[k][good]) == bits(full[k][[ids[i] for i in good]])).all(), k
        assert np.isnan(by_id[k][[3, 6]]).all(), k                             # left as they were
    # the same call twice; pair_dist alone; one row
    again = gpu_query(core, N)
    alone = gpu_query(core, N, want=("pair_dist",))
    one = gpu_query(core, 1, env_ids=[37], want=("self_min", "cap_env"))
    for k in ALL:
        assert (bits(again[k]) == bits(full[k])).all(), k
    assert (bits(alone["pair_dist"]) == bits(full["pair_dist"])).all()
    assert (bits(one["self_min"]) == bits(full["self_min"][[37]])).all() and (bits(one["cap_env"]) == bits(full["cap_env"][[37]])).all()
    # a q override of 130 rows (three workgroups): every row is its own problem
    rep = np.concatenate([np.arange(N), np.arange(60)])
    big = gpu_query(core, len(rep), q=q[rep], box=box[rep])
    for k in ALL:
        assert (bits(big[k]) == bits(full[k][rep])).all(), k
    # purity
    assert _same(before, _snapshot(core))
    state1 = env.get_state()
    assert state0.stamp == state1.stamp and all(torch.equal(getattr(state0, n), getattr(state1, n)) for n in ("bank", "stats", "counters", "actions"))
    # the argument errors that need a live handle
    lib, h = core.lib, core.h
    buf = torch.zeros(N, NP, device=core.device)
    p = C.c_void_p(buf.data_ptr())
    assert lib.dexsim_query_proximity(h, None, N - 1, None, None, 0.0, None, None, p, None) == 1
    assert b"k == num_envs" in lib.dexsim_last_error()
    h2 = C.c_void_p()
    sc, ms = _setup(N)
    assert lib.dexsim_create(C.byref(sc), C.byref(ms), core.dev_index, C.byref(h2)) == 0
    assert lib.dexsim_query_proximity(h2, None, N, None, None, 0.0, None, None, p, None) == 2   # DEXSIM_ERR_NOT_BOUND
    ms.cap_fslot[4] = 2                                                        # a second capsule on the thumb's distal link
    h3 = C.c_void_p()
    assert lib.dexsim_create(C.byref(sc), C.byref(ms), core.dev_index, C.byref(h3)) == 0
    assert lib.dexsim_query_proximity(h3, None, N, None, None, 0.0, None, None, p, None) == 1
    assert b"one capsule per finger link" in lib.dexsim_last_error()
    assert lib.dexsim_destroy(h2) == 0 and lib.dexsim_destroy(h3) == 0
    torch.cuda.synchronize()
    assert not buf.any()                                                       # none of them launched
    env.close()


@pytest.mark.gpu
def test_no_box(hp, poses):
    from dexrobot_isaac_amd.core import DexSimCore
    sc, ms = _setup(N, "BaseTask")
    assert not sc.has_box
    core = DexSimCore(sc, ms, "cuda:0")
    core.reset()
    q = poses["q"]
    pose_core(core, q)
    ref = _reference(hp, q, None)
    empty = np.zeros(8, np.float32)
    empty[0] = np.inf
    state = gpu_query(core, N)
    assert (bits(state["cap_env"][:, :, 0]) == bits(empty)).all()              # (+inf, 0, ...)
    _check_against(state, ref, box=False, label="no box: ")
    over = gpu_query(core, N, q=q)
    for k in ALL:
        assert (bits(over[k]) == bits(state[k])).all(), k
    # a box_pose override: the box_size argument is honoured
    for size in (0.04, 0.09):
        refb = _reference(hp, q, poses["box"], size)
        for kw in (dict(q=q), dict()):                                         # with the q override and on the state path
            out = gpu_query(core, N, box=poses["box"], size=size, **kw)
            _check_against(out, refb, label=f"box_size {size}: ")
    core.close()


# ------------------------------------------------------------------------------------------------- against the engine's narrowphase
def _narrowphase_states(hp, co, rng):
    """70 states (q (N, 26), box (N, 7), chosen capsule, record: 0 box, 1 ground): rows 0-57 bring the tip end of a chosen capsule to within
    U(-0.5, 2) mm of a face of the box with every other capsule clear of it and the hand clear of the ground; rows 58-69 bring
    the lowest capsule end to within that of the ground with the box far away."""
    geom, hb = hp.geom, 0.5 * hp.box_size
    q_all, _ = hp.test_poses(4 * N, SEED + 1)
    zj = int(np.argmax([abs(geom.fk(np.eye(NJ)[j])[0][5][2] - geom.fk(np.zeros(NJ))[0][5][2]) for j in range(3)]))   # the z slide
    zs = 1.0 / (geom.fk(np.eye(NJ)[zj])[0][5][2] - geom.fk(np.zeros(NJ))[0][5][2])   # slide per metre of height: +-1 where its axis is vertical
    qs, boxes, caps, kinds = [], [], [], []
    tries = iter(range(len(q_all)))
    while len(qs) < N:
        q = q_all[next(tries)].astype(np.float64)
        row = len(qs)
        a, b, _ = hp.capsules(q[None], np.float64)
        low = np.minimum(a[0, :, 2], b[0, :, 2]) - hp.r
        gap = rng.uniform(-0.5e-3, 2e-3)
        if row >= 58:                                                          # ground row: the lowest end at `gap`
            q[zj] += zs * (gap - low.min())
            box = np.array([1.0, 1.0, 1.0, 0, 0, 0, 1.0])
            qs.append(q), boxes.append(box), caps.append(int(np.argmin(low))), kinds.append(1)
            continue
        q[zj] += zs * (0.25 - low.min())                                       # box row: the hand well above the ground
        a, b, _ = hp.capsules(q[None].astype(np.float32), np.float64)
        c = int(rng.integers(3, NCAP))
        tip, ax = b[0, c], b[0, c] - a[0, c]
        u = ax / np.linalg.norm(ax)
        for _ in range(40):                                                    # a face that tilts away from the axis: the tip is the nearest point
            w = rng.normal(size=3)
            w -= (w @ u) * u
            z = -(np.cos(0.35) * w / np.linalg.norm(w) + np.sin(0.35) * u)     # outward normal of the touched face: from the box to the tip
            x = rng.normal(size=3)
            x -= (x @ z) * z
            x /= np.linalg.norm(x)
            Rb = np.stack([x, np.cross(z, x), z], 1)                           # world <- box; the touched face is the box's +z face
            w4 = 0.5 * np.sqrt(max(1 + np.trace(Rb), 0.0))
            if w4 < 0.1:
                continue
            lat = rng.uniform(-0.6 * hb, 0.6 * hb, size=2)
            centre = tip - Rb @ np.array([lat[0], lat[1], hb + hp.r[c] + gap])
            quat = np.array([Rb[2, 1] - Rb[1, 2], Rb[0, 2] - Rb[2, 0], Rb[1, 0] - Rb[0, 1], 4 * w4 * w4]) / (4 * w4)
            box = np.concatenate([centre, quat / np.linalg.norm(quat)])
            rec, _ = hp.box(a, b, box[None].astype(np.float32))
            others = np.delete(rec[0, :, 0], c)
            if others.min() > co + 2e-3 and abs(rec[0, c, 0] - gap) < 1e-4:
                qs.append(q), boxes.append(box), caps.append(c), kinds.append(0)
                break
    return np.array(qs, np.float32), np.array(boxes, np.float32), np.array(caps), np.array(kinds)


@pytest.mark.gpu
def test_against_engine_narrowphase(hp, poses):
    """The engine's own manifold (stand-alone k_dynamics) against the query of the same state.  D = gap + rest_offset is the engine's
    raw gap of a sample-0 hand / box entry, Q the queried distance of the same capsule, L its axis length, tol the distance bound
    of test_against_reference.  The engine's t is a 2^-10 bisection snapped to an end within 2 %, and distance is 1-Lipschitz in
    the axis point: Q <= D + tol and D - Q <= (0.02 + 2^-11) L + tol."""
    _engine_narrowphase(hp, poses, None)


@pytest.mark.gpu
def test_structure_free_model_engine_narrowphase(hp_generic, poses_generic):
    """The same on the model of tests/generic_model.py: the step path's narrowphase sees capsules that start off the joint origin
    and end off the x axis, on tilted frames."""
    _engine_narrowphase(hp_generic, poses_generic, "generic")


def _engine_narrowphase(hp, poses, model):
    from tests.hip_backend import HipBackend
    sc, ms = _setup(N, model=model)
    co, rest = float(sc.contact_offset), float(sc.rest_offset)
    rng = np.random.default_rng(SEED + 2)
    q, box, chosen, kinds = _narrowphase_states(hp, co, rng)
    hb = HipBackend(sc, ms, "cuda:0", fused=False)
    hb.reset()
    hb.set("q", q.T), hb.set("qd", 0.0)
    hb.set("box_pos", box[:, :3].T), hb.set("box_quat", box[:, 3:].T), hb.set("box_lin", 0.0), hb.set("box_ang", 0.0)
    core = hb.core
    assert (core.field("q").t().cpu().numpy() == q).all() and (core.field("box_quat").t().cpu().numpy() == box[:, 3:]).all()
    core.run_stage(_abi.STAGE["DYNAMICS"])
    out = gpu_query(core, N, want=("cap_env",))["cap_env"].astype(np.float64)
    ncontact = hb.get("ncontact")[0].astype(int)
    codes = hb.get("ccode").astype(int)
    a, b, _ = hp.capsules(q, np.float64)
    L = np.linalg.norm(b - a, axis=-1)
    slack = 0.02 + 2.0 ** -11
    tol_b, tol_g = poses["tol"]["box_d"], poses["tol"]["ground_d"]
    assert ncontact.max() <= 12, "a state lists more than 12 contacts"
    with_box, worst = 0, dict(q_above_d=-np.inf, d_above_q=-np.inf, ground=0.0)
    checked = 0
    for e in range(N):
        con = hb.contacts(e)
        sample = (codes[:ncontact[e], e] >> 7) & 7
        hand_box = con[:, 8] == 1
        with_box += bool(hand_box.any())
        for c in range(NCAP):
            mine = con[:, 9] == c
            # ---- the box
            Q = out[e, c, 0, 0]
            if Q > -hp.r[c]:                                                   # the axis does not meet the box
                s0 = con[mine & hand_box & (sample == 0)]
                assert len(s0) <= 1
                if len(s0):
                    D = s0[0, 6] + rest
                    worst["q_above_d"], worst["d_above_q"] = max(worst["q_above_d"], Q - D), max(worst["d_above_q"], D - Q - slack * L[e, c])
                    assert Q <= D + tol_b, (e, c, Q, D)                        # Q is the minimum
                    assert D - Q <= slack * L[e, c] + tol_b, (e, c, Q, D)
                    checked += 1
                if Q < co - slack * L[e, c] - tol_b:
                    assert len(s0) == 1, (e, c, Q)
                if Q > co + tol_b:
                    assert not (mine & hand_box).any(), (e, c, Q)
            # ---- the ground
            G = out[e, c, 1, 0]
            gr = con[mine & (con[:, 8] == 0)]
            if len(gr):
                worst["ground"] = max(worst["ground"], abs((gr[:, 6] + rest).min() - G))
                assert abs((gr[:, 6] + rest).min() - G) <= tol_g, (e, c, G, gr[:, 6] + rest)
            if G < co - tol_g:
                assert len(gr) >= 1, (e, c, G)
            if G > co + tol_g:
                assert len(gr) == 0, (e, c, G)
    print(f"{with_box} of {N} envs list a hand / box contact, {checked} sample-0 entries compared; Q - D <= {worst['q_above_d']:.3g} (bound {tol_b:.3g}), "
          f"D - Q - (0.02 + 2^-11) L <= {worst['d_above_q']:.3g} (bound {tol_b:.3g}); ground entries off the record by <= {worst['ground']:.3g} "
          f"(bound {tol_g:.3g})")
    assert with_box >= 30
    # the chosen capsule is where it was put: the query sees the constructed gap
    for e in range(N):
        rec = out[e, chosen[e], kinds[e]]
        assert -0.6e-3 <= rec[0] <= 2.1e-3, (e, chosen[e], kinds[e], rec[0])
    core.close()
