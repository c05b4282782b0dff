"""Physics of the oracle (= the specification the HIP integrator implements).  There is no PhysX ground truth
(parity vs PhysX: UNPINNED), so the oracle is checked against first principles:
mass matrix / gravity / Coriolis against numerical differentiation of the kinematics, static equilibrium,
resting contact, frictional pushing, and fp32-vs-fp64 agreement that sizes the GPU parity tolerances."""
import numpy as np
import pytest

from dexrobot_isaac_amd.config import build_sim_config, default_cfg
from oracle.oracle import Oracle


def _mk(task="BlindGrasping", n=4, f64=False):
    cfg = default_cfg(task)
    cfg["env"]["numEnvs"] = n
    sc, model = build_sim_config(cfg)
    return Oracle(sc, model.to_struct(), f64=f64), model, sc


def _numeric_mass_and_gravity(model, q, eps=1e-6):
    m = model

    def parent(j):
        return -1 if j == 0 else (j - 1 if j < 6 else (5 if (j - 6) % 4 == 0 else j - 1))

    def rodr(ax, a):
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K

    def fk(q):
        R, o = [None] * 26, [None] * 26
        for j in range(26):
            p = parent(j)
            Rp, op = (m.spawn_rot, m.spawn_pos) if p < 0 else (R[p], o[p])
            Rz, oj = Rp @ m.jRoff[j], op + Rp @ m.jpoff[j]
            if m.jtype[j] == 0:
                R[j], o[j] = Rz, oj + Rz @ m.jaxis[j] * q[j]
            else:
                R[j], o[j] = Rz @ rodr(m.jaxis[j], q[j]), oj
        return np.array([o[j] + R[j] @ m.com[j] for j in range(26)]), R

    def sym(s):
        return np.array([[s[0], s[3], s[4]], [s[3], s[1], s[5]], [s[4], s[5], s[2]]])

    c0, R0 = fk(q)
    Jv, Jw = np.zeros((26, 3, 26)), np.zeros((26, 3, 26))
    for k in range(26):
        dq = np.zeros(26)
        dq[k] = eps
        c1, R1 = fk(q + dq)
        c2, R2 = fk(q - dq)
        Jv[:, :, k] = (c1 - c2) / (2 * eps)
        for j in range(26):
            dR = (R1[j] - R2[j]) / (2 * eps) @ R0[j].T
            Jw[j, :, k] = [dR[2, 1], dR[0, 2], dR[1, 0]]
    M = sum(m.mass[j] * Jv[j].T @ Jv[j] + Jw[j].T @ (R0[j] @ sym(m.inertia[j]) @ R0[j].T) @ Jw[j] for j in range(26))
    V = lambda qq: float(np.sum(m.mass * 9.81 * fk(qq)[0][:, 2]))
    g = np.array([(V(q + np.eye(26)[k] * eps) - V(q - np.eye(26)[k] * eps)) / (2 * eps) for k in range(26)])
    return M, g


def _derivation_poses():
    """The original pose, and rows of tests/wide_states.py: the whole joint range at speed, base rotations and the first thumb joint
    outside quadrant 0 of the half-angle -- where tests/test_wide_poses.py uses M and b."""
    from tests import wide_states
    rng = np.random.default_rng(0)
    poses = [(rng.uniform(-0.3, 0.6, 26), rng.uniform(-1, 1, 26))]
    st = wide_states.sample("free")
    thumb_far = int(np.argmax(st["q"][6]))
    assert st["q"][6, thumb_far] > np.pi / 2 and (np.abs(st["q"][3:6, :4]) > np.pi / 2).any()
    return poses + [(st["q"][:, e].copy(), st["qd"][:, e].copy()) for e in (0, 1, 2, 3, thumb_far)]


def test_mass_matrix_gravity_coriolis_match_numerical_derivation():
    o, model, _ = _mk(f64=True)
    for q, qd in _derivation_poses():
        _check_derivation(o, model, q, qd)


def test_mass_matrix_gravity_coriolis_match_numerical_derivation_on_the_generic_model():
    """The same derivation on the hand model without exact zeros, ones and repeated numbers (tests/generic_model.py, through
    tests/physics_rig.py): the original pose, rows of the wide sample drawn for this model's limits, and four poses over the full
    joint range -- the oracle is the reference of every GPU test that runs on this model."""
    from tests import physics_rig, wide_states
    sc, model, ms = physics_rig.setup("BlindGrasping", 4, model="generic")
    o = Oracle(sc, ms, f64=True)
    scN, modelN, _ = physics_rig.setup("BlindGrasping", physics_rig.N, model="generic")
    st = wide_states.sample("free", physics_rig.N, physics_rig.SEED, config=(scN, modelN))
    rng = np.random.default_rng(0)
    poses = [(rng.uniform(-0.3, 0.6, 26), rng.uniform(-1, 1, 26))] + [(st["q"][:, e].copy(), st["qd"][:, e].copy()) for e in (0, 1, 2, 3)]
    poses += [(rng.uniform(model.lo, model.hi), rng.uniform(-1, 1, 26)) for _ in range(4)]
    for q, qd in poses:
        _check_derivation(o, model, q, qd)


def _check_derivation(o, model, q, qd):
    M, b0 = o.mass_matrix(q, np.zeros(26))
    Mn, gn = _numeric_mass_and_gravity(model, q)
    assert np.abs(M - Mn).max() < 1e-7 and np.abs(M - M.T).max() == 0 and np.linalg.eigvalsh(M).min() > 0
    assert np.abs(b0 - gn).max() < 1e-6
    _, b = o.mass_matrix(q, qd)
    e = 1e-5
    Mof = lambda qq: o.mass_matrix(qq, np.zeros(26))[0]
    Mdot = (Mof(q + e * qd) - Mof(q - e * qd)) / (2 * e)
    dT = np.array([(qd @ Mof(q + np.eye(26)[k] * e) @ qd - qd @ Mof(q - np.eye(26)[k] * e) @ qd) / (2 * e) for k in range(26)])
    assert np.abs((b - b0) - (Mdot @ qd - 0.5 * dT)).max() < 1e-8      # c(q, qd) = Mdot qd - 1/2 d(qd' M qd)/dq


def test_hand_base_mount_is_90deg_about_y():
    o, model, _ = _mk()
    o.publish()
    hp = o.get("site_pose")[:7, 0]
    np.testing.assert_allclose(hp[:3], [0, 0, 0.5], atol=1e-7)                   # spawn (cfg initialHandPos)
    np.testing.assert_allclose(hp[3:], [0, np.sqrt(0.5), 0, np.sqrt(0.5)], atol=1e-6)   # observation_encoder.py:1496-1503
    tips = o.get("site_pose")[7:42, 0].reshape(5, 7)
    assert (tips[1:, 2] < 0.4).all()                                             # fingers point down (-z)


def test_static_equilibrium_and_resting_box():
    o, _, sc = _mk(n=2)
    z = np.zeros((2, 18), dtype=np.float32)
    o.set("targets", 0.0)
    for _ in range(100):
        o.physics_step()
    q, qd = o.get("q"), o.get("qd")
    assert abs(q[2, 0] + 0.5268 * 9.81 / 10000) < 2e-5                          # ARTz sags by m g / kp
    assert np.abs(qd).max() < 1e-4
    bp, bl = o.get("box_pos"), o.get("box_lin")
    assert abs(bp[2, 0] - (0.025 + sc.rest_offset)) < 1e-4 and np.abs(bl).max() < 1e-4
    np.testing.assert_allclose(o.get("cforce")[48:51, 0], [0, 0, 0.1 * 9.81], atol=1e-3)   # ground reaction = m g
    assert (o.get("ncontact")[0] == 4).all()


def test_fingers_press_on_box():
    """Lower the hand at the task's base speed limit (0.1 m/s) until the fingertips press on the box top: the
    box must stay on the ground (no tunnelling either way), the ground reaction must carry the extra load, and the
    distal links must report contact forces (the source of the obs path's contact_binary)."""
    o, _, sc = _mk(n=1)
    tg = np.zeros((26, 1))
    for _ in range(300):
        tg[2] = max(tg[2] - 0.001, -0.2445)      # ARTz target: middle fingertip sphere ~2 mm into the box top
        o.set("targets", tg)
        o.physics_step()
    cf = o.get("cforce")[:, 0].reshape(17, 3)
    distal = np.linalg.norm(cf[[2, 5, 8, 11, 14]], axis=1)
    assert o.get("ncontact")[0, 0] > 4
    assert distal.max() > 1.0 and distal.max() < 60.0          # ~ kp * penetration demand, not an explosion
    assert abs(o.get("box_pos")[2, 0] - 0.0255) < 3e-3 and np.abs(o.get("box_lin")).max() < 0.05
    tips = o.get("site_pose")[7:42, 0].reshape(5, 7)
    assert tips[1:4, 2].min() > 0.05 + 0.007 - 4e-3             # tip spheres rest on the box top (z = 0.0505)
    assert np.isfinite(o.get("q")).all() and np.abs(o.get("qd")).max() < 1.0


def test_fp32_oracle_agrees_with_fp64_oracle():
    """Sizes the GPU parity tolerance: a single control step of the fp32 oracle vs the fp64 oracle."""
    o32, _, _ = _mk(n=16)
    o64, _, _ = _mk(n=16, f64=True)
    o32.reset()
    o64.reset()
    rng = np.random.default_rng(1)
    for _ in range(5):
        a = (2 * rng.random((16, 18)) - 1).astype(np.float32)
        ob32, _, _ = o32.step(a)
        ob64, _, _ = o64.step(a)
    assert np.abs(ob32 - ob64).max() < 2e-3
    assert np.median(np.abs(ob32 - ob64)) < 1e-6


def test_philox_reset_stream_is_reproducible_and_uniform():
    o, _, _ = _mk(n=512)
    o.reset()
    q = o.get("q")
    box = o.get("initial_box_pos")
    assert np.abs(box[0]).max() <= 0.02 + 1e-7 and np.abs(box[1]).max() <= 0.02 + 1e-7 and (box[2] == np.float32(0.027)).all()
    assert abs(box[0].mean()) < 0.003 and box[0].std() > 0.009                  # U(-0.02, 0.02): std 0.0115
    o2, _, _ = _mk(n=512)
    o2.reset()
    assert np.array_equal(o2.get("initial_box_pos"), box)                        # same (seed, env, reset_count) key
    o2.reset()
    assert not np.array_equal(o2.get("initial_box_pos"), box)                    # next reset_count -> new draw


def test_narrowphase_properties_of_the_round2_manifold():
    """The contact manifold's specification (closest feature, <= 2 per capsule / box pair, <= 4 box / ground corners,
    DEXSIM_KMAX entries) as properties of the lists the oracle produces, over a spread of hand poses on and around the box:
    every contact point lies on the surface it claims, normals are unit and point from the box / the ground into the hand
    body, gaps are consistent with the geometry, the list order is box/ground first, and no capsule has more than two box
    contacts and two ground contacts."""
    from dexrobot_isaac_amd import _abi
    n = 64
    o, model, sc = _mk(n=n, f64=True)
    rng = np.random.default_rng(4)
    q = np.zeros((26, n))
    q[2] = rng.uniform(-0.46, -0.30, n)
    q[:2] = rng.uniform(-0.03, 0.03, (2, n))
    q[3:6] = rng.uniform(-0.2, 0.2, (3, n))
    q[6:] = rng.uniform(0.0, 0.6, (20, n))
    yaw = rng.uniform(-np.pi, np.pi, n)
    o.set("q", q); o.set("qd", 0 * q); o.set("targets", q)
    o.set("box_pos", np.stack([0 * yaw, 0 * yaw, 0.025 + 0 * yaw]))
    o.set("box_quat", np.stack([0 * yaw, 0 * yaw, np.sin(yaw / 2), np.cos(yaw / 2)]))
    o.set("box_lin", np.zeros((3, n))); o.set("box_ang", np.zeros((3, n)))
    bq, bp = o.get("box_quat").copy(), o.get("box_pos").copy()          # the pose the narrowphase sees (start of the sub-step)
    o.substep(last=True)
    hb = 0.5 * float(sc.box_size)
    co, rest = float(sc.contact_offset), float(sc.rest_offset)
    seen_two, total = 0, 0
    for e in range(n):
        c = o.contacts(e)
        total += len(c)
        assert len(c) <= _abi.KMAX
        types = c[:, 8].astype(int)
        nbg = int((types == 2).sum())
        assert nbg <= 4 and (types[:nbg] == 2).all() and (types[nbg:] != 2).all()      # box/ground first, at most 4
        np.testing.assert_allclose(np.linalg.norm(c[:, 3:6], axis=1), 1.0, atol=1e-9)
        s, cq = bq[2, e], bq[3, e]                                       # yaw-only box orientation
        R = np.array([[cq * cq - s * s, -2 * s * cq, 0], [2 * s * cq, cq * cq - s * s, 0], [0, 0, 1.0]])
        for row in c:
            p, nrm, gap, typ = row[0:3], row[3:6], row[6], int(row[8])
            assert gap < co - rest + 1e-12                               # only contacts inside the contact offset are listed
            if typ in (0, 2):                                            # on the ground plane, normal +z
                np.testing.assert_allclose(nrm, [0, 0, 1], atol=1e-12)
                if typ == 0:
                    assert abs(p[2] - (gap + rest)) < 1e-9               # the point is the capsule's lowest point: z = gap + rest
            else:                                                        # on the box surface
                pl = R.T @ (p - bp[:, e])
                assert np.max(np.abs(pl)) <= hb + 1e-9 and (np.abs(np.abs(pl) - hb) < 1e-9).any()
                nl = R.T @ nrm
                assert np.dot(nl, pl) > 0                                # outward
        for cap in range(_abi.NCAP):
            mine = c[(types != 2) & (c[:, 9] == cap)]
            assert (mine[:, 8] == 1).sum() <= 2 and (mine[:, 8] == 0).sum() <= 2
            seen_two += int((mine[:, 8] == 1).sum() == 2)
    assert total > 6 * n and seen_two > 0                                # the sample has line contacts (two points on one capsule)


def test_warm_started_block_solver_reaches_the_converged_solution():
    """Round 2's contact solver (warm start + block-parallel projected Gauss-Seidel with mass splitting, 16 sweeps per
    sub-step) against the same solver run to convergence (200 sweeps): one finger pressing the box onto the ground -- a
    stack, the hard case for a Jacobi-type scheme.  Once the contact persists the 16-sweep solver carries the converged
    impulses from sub-step to sub-step: same contact force, box at rest.  (Round 1's cold-started sequential solver
    left 26 N of these 30 N and a box creeping at 1 cm/s.)  The warm-start cache itself: one generation per sub-step, one
    valid slot per contact."""
    def run(iters):
        cfg = default_cfg("BlindGrasping")
        cfg["env"]["numEnvs"] = 1
        sc, model = build_sim_config(cfg)
        sc.num_position_iterations = iters
        o = Oracle(sc, model.to_struct(), f64=True)
        tg = np.zeros((26, 1))
        for _ in range(300):
            tg[2] = max(tg[2] - 0.001, -0.2445)
            o.set("targets", tg)
            o.physics_step()
        cf = o.get("cforce")[:, 0].reshape(17, 3)
        return o, np.linalg.norm(cf[8]), np.abs(o.get("box_lin")).max(), np.abs(o.get("box_ang")).max()
    o16, f16, v16, w16 = run(16)
    _, f200, v200, _ = run(200)
    assert 20.0 < f200 < 40.0 and v200 < 1e-8                   # the converged solution: ~30 N on the middle fingertip, box at rest
    assert abs(f16 - f200) < 1e-3 * f200 and v16 < 1e-8 and w16 < 1e-8
    gen, tag, nc = int(o16.get("wgen")[0, 0]), o16.get("wtag")[:, 0].astype(int), int(o16.get("ncontact")[0, 0])
    assert gen == 300 * 4 and ((tag >> 3) == gen).sum() == nc    # 4 box/ground slots + the fingertip contact
    assert nc == 5 and (tag[80:84] >> 3 == gen).all() and sorted(tag[80:84] & 7) == [0, 1, 2, 3]   # bottom corners of the box


def test_warm_start_generation_wraps_without_losing_the_cache():
    """the warm-start generation only ever grows (one per sub-step, one per reset) and the cache tags are
    8 * generation + corner in signed 32-bit arithmetic.  It now wraps at 2^27 (DEXSIM_WGEN_NEXT): an env whose generation
    crosses the wrap while a finger presses on the box must go through exactly the same states as one far away from it -- the
    cache keeps warming across the wrap, and no tag ever leaves the positive int range (UBSan build: make -C oracle asan)."""
    def run(gen0):
        o, _, _ = _mk(n=1, f64=True)
        tg = np.zeros((26, 1))
        for s in range(300):
            if s == 260:                         # contact established: move the generation to gen0 (tags move with it)
                g = int(o.get("wgen")[0, 0])
                tag = o.get("wtag")[:, 0].astype(np.int64)
                o.set("wtag", np.where(tag >> 3 == g, 8 * gen0 + (tag & 7), 0).reshape(-1, 1))
                o.set("wgen", np.array([[gen0]]))
            tg[2] = max(tg[2] - 0.001, -0.2445)
            o.set("targets", tg)
            o.physics_step()
        return o
    wrap = 1 << 27
    a, b = run(1000), run(wrap - 40)             # 40 physics steps x 4 sub-steps = 160 generations: b crosses the wrap
    assert int(a.get("wgen")[0, 0]) == 1000 + 160 and int(b.get("wgen")[0, 0]) == (wrap - 40 + 160) % wrap == 120
    for f in ("q", "qd", "box_pos", "box_lin", "cforce", "wlam"):
        np.testing.assert_array_equal(a.get(f), b.get(f), err_msg=f)
    tb, gb = b.get("wtag")[:, 0].astype(np.int64), int(b.get("wgen")[0, 0])
    assert ((tb >> 3) == gb).sum() == int(b.get("ncontact")[0, 0]) == 5 and tb.min() >= 0 and tb.max() < (1 << 30)
    assert np.linalg.norm(b.get("cforce")[:, 0].reshape(17, 3)[8]) > 20.0      # still the converged ~30 N press


def _limit_cfg(rows, n=1, iters=16, f64=True):
    cfg = default_cfg("BlindGrasping")
    cfg["env"]["numEnvs"] = n
    cfg["sim"]["dexsim_joint_limit_rows"] = rows
    cfg["sim"]["physx"]["num_position_iterations"] = iters
    sc, model = build_sim_config(cfg)
    return Oracle(sc, model.to_struct(), f64=f64), model, sc


def test_joint_limit_rows_option():
    """sim.dexsim_joint_limit_rows (round 3, VERDICT missing #3): joint limits as unilateral rows of the contact solver -- for the
    fingers that touch something, every joint within the margin of a limit gets a one-row speculative constraint (a block of its
    own).  (a) Without contacts the option changes nothing, bit for bit.  (b) A straight middle finger pressed onto the box with
    the hand tilted so that the contact force loads the PIP / DIP joints against their lower stops (lo = 0): the rows of
    exactly those joints carry positive impulses, the joints sit ON the limit at rest (no clamp needed), rows of unloaded joints
    carry none (complementarity); the list is 4 box/ground + 1 contact + the finger's 4 lower-limit rows; the rows are neither
    contacts in the statistics nor forces on a body; 16 warm-started sweeps are within 15 % of the converged impulses."""
    # (a) free space
    a, _, _ = _limit_cfg(0, n=4)
    b, _, _ = _limit_cfg(1, n=4)
    a.reset(), b.reset()
    rng = np.random.default_rng(0)
    for _ in range(5):
        act = (2 * rng.random((4, 18)) - 1).astype(np.float32)
        oa, _, _ = a.step(act)
        ob, _, _ = b.step(act)
    np.testing.assert_array_equal(oa, ob)
    # (b) the loaded stop
    def run(rows, iters):
        o, model, sc = _limit_cfg(rows, iters=iters)
        o.set("box_pos", np.array([[0.0], [0.0], [0.0255]]))
        q = np.zeros((26, 1))
        q[4], q[0] = 0.4, 0.08
        o.set("q", q)
        tg = q.copy()
        for _ in range(500):
            tg[2] = max(tg[2, 0] - 0.001, -0.275)
            o.set("targets", tg)
            o.physics_step()
        return o, model
    o, model = run(1, 16)
    oc, _ = run(1, 200)
    K = int(o.get("ncontact")[0, 0])
    con = o.contacts(0)
    assert K == 9 and list(con[:, 8].astype(int)) == [2, 2, 2, 2, 1, 3, 3, 3, 3] and list(con[5:, 9].astype(int)) == [0, 1, 2, 3]
    np.testing.assert_allclose(con[5:, 6], o.get("q")[14:18, 0] - model.lo[14:18], atol=1e-6)     # gap = distance to the lower limit
    lam = o.get("wlam")[:, 0].reshape(-1, 3)
    lamc = oc.get("wlam")[:, 0].reshape(-1, 3)
    keys = [88 + (8 + l) * 2 for l in range(4)]                     # finger 2, joints 0..3, lower side
    tag, gen = o.get("wtag")[:, 0].astype(int), int(o.get("wgen")[0, 0])
    assert all(tag[k] >> 3 == gen for k in keys)
    q, qd = o.get("q")[14:18, 0], o.get("qd")[14:18, 0]
    loaded = lam[keys, 0] > 1e-4
    assert list(loaded) == [False, True, True, True]                # spread joint unloaded; MCP flexion, PIP, DIP on their stops
    assert np.abs(q[loaded] - model.lo[14:18][loaded]).max() < 1e-7 and np.abs(qd[loaded]).max() < 1e-6
    assert (lam[keys, 1:] == 0).all() and (lam[keys, 0] >= 0).all()
    assert np.abs(lam[keys, 0] - lamc[keys, 0]).max() < 0.15 * lamc[keys, 0].max()
    assert float(o.stats()[19]) == 1.0 and float(o.stats()[18]) == 9.0     # mean hand contacts: the one contact; list length 9
    cf = o.get("cforce")[:, 0].reshape(17, 3)
    assert np.linalg.norm(cf[8]) > 100 and np.abs(np.delete(cf, [8, 16], axis=0)).max() == 0.0   # only the distal link and the box feel a force
    # fp32 oracle agrees with fp64 here too
    o32, _, _ = _limit_cfg(1, f64=False)
    for f in ("q", "qd", "targets", "box_pos", "box_quat", "box_lin", "box_ang", "wlam", "wtag", "wgen"):   # (state + warm-start cache)
        o32.set(f, o.get(f))
    o64 = o
    o32.physics_step(), o64.physics_step()
    np.testing.assert_allclose(o32.get("q"), o64.get("q"), atol=2e-5)
