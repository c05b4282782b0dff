"""The structure-free hand model of tests/generic_model.py, from the references alone (no GPU): it is a model validate_model accepts
and an MJCF file can say, it has none of the default model's zeros, ones and repeated numbers, and every one of those properties
BITES -- the float64 references of the suites, evaluated on the generic model with one property put back to the default's value,
move by at least ten bounds of some quantity.  So a kernel that folds a property away would be refused by the GPU tests that run on
this model (test_structure_free_model of every query suite, the `generic` cases of test_wide_poses and test_model_structure).

The bounds the bite is measured against.  Forward kinematics, Jacobian, scene records: the suites' absolute bounds (fk_ref.POS_TOL,
QUAT_TOL, VEL_TOL, KE_TOL; 1e-5).  Mass matrix, gravity, inverse and forward dynamics, bias acceleration: the CAPS that the suites'
test_reference_roundoff put on FACTOR x the float32 reference's error (1e-4, 1e-5, 1e-3) -- the bounds the GPU tests use are below
them, so ten caps is more than ten bounds.  IK and proximity: 4 x the float32 reference's own error on these rows, as their suites
compute it.  Step path: C_RULE x the fp32 oracle's error on qd after one sub-step plus the floor 1e-6 (physics_rig.assert_c_rule's
rule at the maximum).
"""
import ctypes as C

import numpy as np

from dexrobot_isaac_amd import _abi
from dexrobot_isaac_amd.mjcf import export_mjcf, load_mjcf
from tests import fk_ref, fwddyn_ref, ik_ref, invdyn_ref as ir, kindyn_ref as kr, physics_rig, proximity_ref, wide_states
from tests.query_rig import generic_hand, generic_properties, setup

NJ, NB, NS, NCAP = _abi.NJ, _abi.NUM_HAND_BODIES, _abi.NSITE, _abi.NCAP
ROWS = 24
A = lambda x: np.array(np.ctypeslib.as_array(x), dtype=np.float64)


def _angle(q):
    """Rotation angle of xyzw quaternions (..., 4)."""
    q = np.asarray(q, dtype=np.float64)
    return 2 * np.arctan2(np.linalg.norm(q[..., :3], axis=-1), np.abs(q[..., 3]))


# ------------------------------------------------------------------------------------------------- validity
def test_the_model_is_valid_and_has_no_structure():
    sc, ms = setup(4, model="generic")
    # validate_model's constraints (csrc/dexsim.hip), mirrored
    assert list(ms.jtype) == [0, 0, 0] + [1] * 23
    assert not A(ms.mass)[:5].any() and not A(ms.inertia)[:5].any() and not A(ms.com)[:5].any() and (A(ms.mass)[5:] > 0).all()
    assert list(ms.cap_parent) == [5, 5, 5] + [6 + 4 * f + 1 + l for f in range(5) for l in range(3)]
    assert all(0 <= s < _abi.FSLOT_BOX for s in ms.cap_fslot)
    assert list(ms.site_parent) == [5] + [9 + 4 * f for f in range(5)] * 2
    assert (A(ms.hi) > A(ms.lo)).all()
    default = setup(4)[1]
    assert list(ms.body_parent) == list(default.body_parent) and list(ms.body_fslot) == list(default.body_fslot)
    # no identity, no zero, no axis-aligned direction
    assert _angle(A(ms.jqoff)).min() >= 0.2 and np.abs(A(ms.jpoff)).min() >= 3e-3 and np.abs(A(ms.jaxis)).min() >= 0.05
    assert np.abs(np.linalg.norm(A(ms.jaxis), axis=1) - 1).max() <= 1e-7
    assert np.abs(A(ms.com)[5:]).min() >= 1.5e-3
    I = A(ms.inertia)[5:]
    assert (np.abs(I[:, 3:]).min(1) >= 0.02 * I[:, :3].max(1)).all()
    for j in range(5, NJ):                                                      # a physical tensor: positive definite, triangle inequality
        w = np.linalg.eigvalsh(np.array([[I[j - 5][0], I[j - 5][3], I[j - 5][4]], [I[j - 5][3], I[j - 5][1], I[j - 5][5]], [I[j - 5][4], I[j - 5][5], I[j - 5][2]]]))
        assert w[0] > 0 and w[0] + w[1] >= w[2] * (1 - 1e-6)
    sq = A(ms.spawn_quat)
    assert _angle(sq) >= 0.5 and np.abs(sq[:3] / np.linalg.norm(sq[:3])).min() >= 0.2
    assert _angle(A(ms.site_q)).min() >= 0.2 and np.abs(A(ms.site_p)).min() >= 1.5e-3
    assert np.abs(A(ms.cap_p0)).min() >= 1.5e-3 and np.abs(A(ms.cap_p1)[:, 1:]).min() >= 1.5e-3
    # every per-joint number differs from every other joint's; the variation stays within +-30 %, the limits within 0.05 rad
    for name in ("kp", "kd", "armature"):
        assert len(set(A(getattr(ms, name)).tolist())) == NJ, name
    assert len(set(A(ms.mass)[5:].tolist())) == NJ - 5 and (A(ms.armature) > 0).all()
    for name in ("kp", "kd", "mass"):
        g, d = A(getattr(ms, name)), A(getattr(default, name))
        assert (np.abs(g[d > 0] / d[d > 0] - 1) <= 0.3 + 1e-6).all(), name
    assert np.abs(A(ms.lo) - A(default.lo)).max() <= 0.05 + 1e-6 and np.abs(A(ms.hi) - A(default.hi)).max() <= 0.05 + 1e-6
    assert (A(ms.lo)[6:] < 0).all()                                              # q = 0, where a reset puts the fingers, is in range
    # the palm, pad and tip bodies ride on their sites, the link bodies on their joint frames
    tied = {6: 0, **{7 + 6 * f + 4: 6 + f for f in range(5)}, **{7 + 6 * f + 5: 1 + f for f in range(5)}}
    for b in range(NB):
        if b in tied:
            assert list(ms.body_q[b]) == list(ms.site_q[tied[b]]) and list(ms.body_p[b]) == list(ms.site_p[tied[b]])
        else:
            assert list(ms.body_q[b]) == [0, 0, 0, 1] and list(ms.body_p[b]) == [0, 0, 0]
    # ... and free_body_frames gives every body a frame of its own
    fb = setup(4, model="generic", free_bodies=True)[1]
    assert _angle(A(fb.body_q)).min() >= 0.2 and np.abs(A(fb.body_p)).min() >= 1.5e-3 and list(fb.body_parent) == list(ms.body_parent)
    # M is positive definite at the rows of the tests
    hk = kr.HandKin(ms)
    M64, _ = kr.mass_gravity(kr.oracle_pair(sc, ms)[1], hk.random_poses(ROWS, seed=21))
    assert (np.linalg.eigvalsh(M64) > 0).all() and np.abs(M64 - M64.transpose(0, 2, 1)).max() == 0


def test_mjcf_round_trip():
    """load_mjcf(export_mjcf(model)) is the same struct: exactly in every field the file states as numbers of the struct (the
    generic model holds float32 numbers), to one float32 spacing where the dialect goes through a product -- quaternions (matrix and
    back) and the palm capsules and inertial data (stated in the right_hand_base body's frame)."""
    hand = generic_hand()
    a, b = hand.to_struct(), load_mjcf(export_mjcf(hand)).to_struct()
    exact = ("spawn_pos", "jtype", "jpoff", "jaxis", "mass", "kp", "kd", "armature", "lo", "hi", "site_parent", "site_p", "cap_parent",
             "cap_r", "cap_fslot", "body_parent", "body_p", "body_fslot")
    close = ("spawn_quat", "jqoff", "site_q", "body_q", "com", "inertia", "cap_p0", "cap_p1")
    assert {n for n, _ in a._fields_} == set(exact) | set(close) | {"hand_friction"}
    assert a.hand_friction == b.hand_friction
    for name in exact:
        assert (A(getattr(a, name)) == A(getattr(b, name))).all(), name
    for name in close:
        x, y = A(getattr(a, name)), A(getattr(b, name))
        assert (np.abs(x - y) <= 1.2e-7 * np.maximum(np.abs(x), 2.0 ** -3)).all(), (name, np.abs(x - y).max())
    for name in ("com", "inertia", "cap_p0", "cap_p1"):                         # ... and the finger links' exactly
        assert (A(getattr(a, name))[6 if name in ("com", "inertia") else 3:] == A(getattr(b, name))[6 if name in ("com", "inertia") else 3:]).all(), name


def test_create_refuses_inertial_data_on_the_massless_base_links():
    """validate_model: links 0-4 carry no mass, and the kernels and the oracle take the base's inertial data from link 5 alone, so an
    inertia or a centre of mass there would be silently ignored.  The check runs before any device call."""
    from tests.query_rig import load_lib
    lib = load_lib()
    sc, _ = setup(4)
    for field, idx, text in (("inertia", (3, 0), b"zero inertia"), ("inertia", (0, 4), b"zero inertia"), ("com", (4, 2), b"zero centre of mass")):
        ms = setup(4)[1]
        getattr(ms, field)[idx[0]][idx[1]] = 1e-4
        h = C.c_void_p()
        assert lib.dexsim_create(C.byref(sc), C.byref(ms), 0, C.byref(h)) == 1          # DEXSIM_ERR_ARG
        assert text in lib.dexsim_last_error(), lib.dexsim_last_error()


# ------------------------------------------------------------------------------------------------- every property bites
def _quantities(sc, ms, rows):
    """The float64 references of the suites on the model `ms` at the shared rows: a dict of arrays."""
    q, qd, qdd, tau_in = rows["q"], rows["qd"], rows["qdd"], rows["tau"]
    out = {}
    fk = fk_ref.HandFK(ms, sc)
    out["body"], out["site"], out["hand"] = fk.body_states(q, qd), fk.site_poses(q), fk.site_poses(q, hand_frame=True)
    out["cen"] = fk.centroid(q, qd)
    hk = kr.HandKin(ms)
    out["jac"] = np.stack([hk.jacobian(x.astype(np.float64)) for x in q])
    o64 = kr.oracle_pair(sc, ms)[1]
    out["M"], out["g"] = kr.mass_gravity(o64, q)
    _, b = ir.mass_bias(o64, q, qd)
    out["tau"] = ir.tau_of(out["M"], b, qdd)
    out["acc"] = np.stack([ir.bias_accel(hk, x.astype(np.float64), v.astype(np.float64)) for x, v in zip(q, qd)])
    out["qdd"] = fwddyn_ref.solve64(out["M"], tau_in - b)
    out["qdd_arm"] = fwddyn_ref.solve64(out["M"], tau_in - b, arm=A(ms.armature))
    hik = ik_ref.HandIK(ms, sc)
    kw = dict(free_mask=ik_ref.FINGERS_FREE, iters=1, damping=1e-2, max_step=0.5)
    out["ik"] = hik.solve(rows["ik_q0"], rows["ik_tg"], **kw)[0]
    out["ik_hand"] = hik.solve(rows["ik_q0"], rows["ik_tg_hand"], frame=1, **kw)[0]
    hp = proximity_ref.HandProx(ms, sc)
    r = hp.query(rows["pq"], rows["pbox"])
    out["prox_ground"], out["prox_box"], out["prox_pair"] = r["cap_env"][:, :, 1, 0], r["cap_env"][:, :, 0, 0], r["pair_dist"]
    out["caps"] = np.concatenate([r["a"], r["b"]], axis=1)
    return out


def _step(sc, ms, st, f64):
    from oracle.oracle import Oracle
    o = Oracle(sc, ms, f64=f64)
    physics_rig.load(o, st)
    o.substep(last=True)
    return o.get("qd")


def test_every_structural_property_bites():
    """For each property of generic_properties(): the generic model with only that property put back to the default's value, the
    float64 references of every suite on it and on the generic model, at the same rows; difference / bound per suite.  Each property
    moves at least one quantity by ten bounds, and the ones a kernel family depends on reach that family."""
    sc, ms = setup(ROWS, model="generic", free_bodies=True)
    hik, hp = ik_ref.HandIK(ms, sc), proximity_ref.HandProx(ms, sc)
    fk = fk_ref.HandFK(ms, sc)
    q, qd = fk.test_rows(ROWS, seed=21, still_base=8)
    _, qdd = ir.random_rates(ROWS, seed=31)
    M64, b64 = ir.mass_bias(kr.oracle_pair(sc, ms)[1], q, qd)
    tau = fwddyn_ref.targets(M64, b64, 41)[1].astype(np.float64)
    _, ik_q0, ik_tg = hik.test_poses(ROWS, 11)
    hand_p, hand_R = hik.hand_frame(hik.u0_of_q(ik_q0))
    ik_tg_hand = np.einsum("nji,nfj->nfi", hand_R, ik_tg.astype(np.float64) - hand_p[:, None, :]).astype(np.float32)
    pq, pbox = hp.test_poses(ROWS, proximity_ref.SEED)
    rows = dict(q=q, qd=qd, qdd=qdd, tau=tau, ik_q0=ik_q0, ik_tg=ik_tg, ik_tg_hand=ik_tg_hand, pq=pq, pbox=pbox)
    G = _quantities(sc, ms, rows)
    # the bounds that are multiples of the float32 reference's own error on these rows of this model
    kw = dict(free_mask=ik_ref.FINGERS_FREE, iters=1, damping=1e-2, max_step=0.5)
    b_ik = 4 * np.abs(hik.solve(ik_q0, ik_tg, dtype=np.float32, **kw)[0].astype(np.float64) - G["ik"]).max()
    b_ikh = 4 * np.abs(hik.solve(ik_q0, ik_tg_hand, frame=1, dtype=np.float32, **kw)[0].astype(np.float64) - G["ik_hand"]).max()
    ptol = proximity_ref.reference(hp, pq, pbox)["tol"]
    # the step path: one sub-step of the oracles from a wide state of this model (the struct without free body frames: the step reads none)
    scs, _, mss = physics_rig.setup("BlindGrasping", ROWS, model="generic")
    st = {k: v[:, :ROWS] for k, v in wide_states.sample("free", physics_rig.N, physics_rig.SEED,
                                                        config=physics_rig.setup("BlindGrasping", physics_rig.N, model="generic")[:2]).items()}
    v64 = _step(scs, mss, st, True)
    b_step = physics_rig.C_RULE * np.abs(_step(scs, mss, st, False) - v64).max() + 1e-6
    must = {"cap_p0 zero on the fingers": {"proximity", "render"}, "cap_p1 on the x axis": {"proximity", "render"},
            "site_q identity on tips and pads": {"fk sites"}, "site 0 on the palm joint's origin": {"fk sites", "ik"},
            "armature zero": {"forward dynamics", "step"}, "body_q, body_p default": {"fk bodies", "jacobian", "inverse dynamics"},
            "kp uniform": {"step"}, "kd uniform": {"step"}, "mass uniform": {"mass matrix", "inverse dynamics", "forward dynamics", "step"},
            "palm products of inertia zero": {"mass matrix", "forward dynamics", "step"}, "base jpoff zero": {"jacobian", "mass matrix", "inverse dynamics"},
            "flexion jqoff identity": {"fk bodies", "jacobian", "mass matrix", "ik", "proximity", "render"},
            "flexion axes -e_y": {"fk bodies", "jacobian", "mass matrix", "ik", "proximity", "render"},
            "flexion jpoff y, z zero": {"fk bodies", "jacobian", "mass matrix", "ik", "proximity", "render"},
            "finger com y, z zero": {"fk centroid", "mass matrix", "inverse dynamics"},
            "spawn identity": {"fk bodies", "jacobian", "mass matrix", "proximity", "render"}}
    assert set(must) <= set(generic_properties())
    mx = lambda e: float(np.max(e[0] / e[1]))
    print()
    for prop in generic_properties():
        scp, msp = setup(ROWS, model="generic", free_bodies=True, restore=prop)
        P = _quantities(scp, msp, rows)
        be, se, he = fk_ref.body_errors(P["body"], G["body"], qd), fk_ref.site_errors(P["site"], G["site"]), fk_ref.site_errors(P["hand"], G["hand"])
        ce = fk_ref.centroid_errors(P["cen"], G["cen"], qd, fk.total_mass, fk.gravity)
        e_lin, e_ang = ir.err_acc(P["acc"], G["acc"])
        handp = fk_ref.HandFK(msp, scp)
        reach = {
            "fk bodies": max(mx(v) for v in be.values()),
            "fk sites": max(max(mx(v) for v in se.values()), max(mx(v) for v in he.values())),
            # (the bound of the potential energy is stated with the total mass: left out where the property changes that mass)
            "fk centroid": max(mx(v) for k, v in ce.items() if k != "potential energy" or abs(handp.total_mass - fk.total_mass) < 1e-12),
            "jacobian": np.abs(P["jac"] - G["jac"]).max() / 1e-5,
            "mass matrix": max(kr.err_M(P["M"], G["M"]) / 1e-4, kr.err_g(P["g"], G["g"], G["M"]) / 1e-5),
            "inverse dynamics": max(ir.err_tau(P["tau"], G["tau"], G["M"]), e_lin, e_ang) / 1e-3,
            "forward dynamics": max(fwddyn_ref.err_qdd(P["qdd"], G["qdd"], G["M"]), fwddyn_ref.err_qdd(P["qdd_arm"], G["qdd_arm"], G["M"])) / 1e-3,
            "ik": max(np.abs(P["ik"] - G["ik"]).max() / b_ik, np.abs(P["ik_hand"] - G["ik_hand"]).max() / b_ikh),
            "proximity": max(np.abs(P["prox_ground"] - G["prox_ground"]).max() / ptol["ground_d"], np.abs(P["prox_pair"] - G["prox_pair"]).max() / ptol["pair_d"],
                             np.abs(P["prox_box"] - G["prox_box"]).max() / ptol["box_d"]),
            "render": np.abs(P["caps"] - G["caps"]).max() / 1e-5,
        }
        if prop != "body_q, body_p default":                                    # (a sub-step's qd reads no body frame)
            msp_step = physics_rig.setup("BlindGrasping", ROWS, model="generic:" + prop)[2]
            reach["step"] = np.abs(_step(scs, msp_step, st, True) - v64).max() / b_step
        hit = sorted(k for k, v in reach.items() if v >= 10)
        print(f"{prop}: " + ", ".join(f"{k} {v:.3g}" for k, v in reach.items()))
        assert hit, f"{prop}: no quantity of any suite moves by ten bounds"
        assert must.get(prop, set()) <= set(hit), f"{prop}: does not reach {sorted(must.get(prop, set()) - set(hit))}"
