"""The box wave and the hand / box narrowphase on TUMBLED boxes (tests/tumbled_states.py), against the fp64 and fp32 oracles.

Every other physics test draws a box that only yaws: it sits on its -z face, the corner list is 0, 1, 2, 3 or empty, a warm-start slot
80 + k never changes its corner, and the hand meets faces.  Here the box rests on one or two corners, on another face or on an edge,
corners leave and move between slots, and most hand / box normals come from an edge or a vertex.

N = 256 envs, seed 11: four workgroups, every box class in each (env i is of class i % 4); the box-alone GPU tests also run on the first
200 envs (last workgroup padded).  The CPU tests show that what the GPU tests rely on holds for the reference alone -- the sample
covers the cases, the two oracles list the same contacts in every env, the oracle's edge / vertex gaps agree with an independent
capsule / box distance -- so that a failing GPU test points at a kernel.

Bounds.  Integers (list length, type, capsule, corner per slot) are exact over the envs whose list length agrees in the fp64 oracle,
the fp32 oracle and the kernels; at most 2 % may be left out (the oracles alone leave out none).  Points and gaps: 2e-6 m, the
project's bound (the fp32 oracle is inside it by 30 x).  Normals: an edge or vertex normal is a normalised difference, its error
goes as 1 / dist with dist = gap + rest_offset + capsule radius (4-8 mm), so the bound is per contact c E / dist + 1e-7 with E the
largest err_n dist of the fp32 oracle against the fp64 oracle on the same sample, computed by the test (3.2e-8 m at N = 256).  States:
the kernels' error against fp64 at the 99.9th percentile and at the maximum is at most c x the fp32 oracle's own error on the same
envs, plus the floors 1e-7 and 1e-6 of test_hip_error_is_a_small_multiple_of_fp32_roundoff, whose c = 3 this file uses throughout.
The references and the comparisons that apply these bounds are in tests/physics_rig.py, shared with the suites that follow this method.
"""
import numpy as np
import pytest

from tests import physics_rig as pr
from tests import tumbled_states as ts

N = pr.N


def _setup(n):
    return pr.setup("BlindGrasping", n)


def _free_ref(n):
    """The box-alone sample free-running for two physics steps (8 sub-steps) on both oracles: snapshots after each step."""
    return pr.tumbled_free_ref("box_alone", n, 2, pr.BOX_FIELDS)


# ------------------------------------------------------------------------------------------------- CPU: the sample and the reference
def _feature_classes(lists, quat):
    """Hand / box entries by the number of non-zero components of the normal in the box frame: face, edge, vertex."""
    R = ts.quat_to_mat(quat.T)
    cls = [0, 0, 0]
    for e, c in enumerate(lists):
        for row in c[c[:, 8] == 1]:
            cls[int((np.abs(R[e].T @ row[3:6]) > 1e-6).sum()) - 1] += 1
    return cls


def test_sample_covers_the_cases():
    """What the fp64 oracle sees in the two samples; every threshold is half of the count observed at N = 256, seed 11."""
    from oracle.oracle import Oracle
    sc, _, ms = _setup(N)
    on, alone = pr.tumbled_teacher_ref("hand_on_box", N)[0], pr.tumbled_teacher_ref("box_alone", N)[0]
    seen = {}
    for name, rec in (("hand_on_box", on), ("box_alone", alone)):
        nbg = np.array([(c[:, 8] == 2).sum() for c in rec["lists64"]])
        assert (nbg == (rec["s64"]["corner"] >= 0).sum(0)).all()          # one valid slot 80 + k per listed corner
        counts = np.bincount(nbg, minlength=5)
        corners = rec["s64"]["corner"]
        other = int(sum(nbg[e] == 4 and set(corners[:, e]) != {0, 1, 2, 3} for e in range(N)))
        seen[name] = dict(counts=counts.tolist(), other=other)
    cls = _feature_classes(on["lists64"], on["start"]["box_quat"])
    hand_ground = int(sum((c[:, 8] == 0).sum() for c in on["lists64"]))
    min_gap = min(c[:, 6].min() for c in on["lists64"] if len(c))
    # corner turnover of the box alone over 8 free-running sub-steps: a valid slot holds another corner, or none, one sub-step later
    o = Oracle(sc, ms, f64=True)
    pr.load(o, pr.tumbled_state("box_alone", N))
    prev, turned, kmax = None, np.zeros(N, bool), 0
    for sub in range(8):
        o.substep(last=sub % 4 == 3)
        _, cur = pr.bg_cache(o)
        if prev is not None:
            turned |= ((prev >= 0) & (cur != prev)).any(0)
        prev, kmax = cur, max(kmax, int(o.get("ncontact").max()))
    print(f"\nbox / ground counts 0-4: {seen}; hand / box face, edge, vertex: {cls}; hand / ground {hand_ground}; min gap {min_gap:.2e}; "
          f"envs with corner turnover {int(turned.sum())}")
    # observed: hand_on_box counts [0, 64, 129, 6, 57], box_alone [57, 51, 101, 3, 44]
    assert seen["hand_on_box"]["counts"][1] >= 32 and seen["hand_on_box"]["counts"][2] >= 64 and seen["hand_on_box"]["counts"][4] >= 28
    assert seen["box_alone"]["counts"][1] >= 25 and seen["box_alone"]["counts"][2] >= 50 and seen["box_alone"]["counts"][4] >= 22
    # observed: four corners other than {0, 1, 2, 3} in 57 and 43 envs
    assert seen["hand_on_box"]["other"] >= 28 and seen["box_alone"]["other"] >= 21
    # observed: 103 face, 127 edge, 30 vertex entries; 57 hand / ground entries; deepest entry -3.2 mm
    assert cls[0] >= 51 and cls[1] >= 63 and cls[2] >= 15 and hand_ground >= 28 and min_gap < -1.6e-3
    # observed: 43 envs
    assert int(turned.sum()) >= 21
    assert kmax <= 4 and max(len(c) for c in on["lists64"]) <= 12        # the box alone: box / ground entries only, the early box solve


def test_both_oracles_list_the_same_contacts():
    """The exclusion rule of the GPU tests leaves out nothing for the reference alone: count, type and capsule agree in every env of
    both samples, over the teacher-forced sub-steps and over the free run; box / ground slots hold the same corners."""
    for kind in ("hand_on_box", "box_alone"):
        recs = pr.tumbled_teacher_ref(kind, N)
        assert all(pr.same_lists(a, b) for a, b in zip(recs[0]["lists64"], recs[0]["lists32"])), kind
        for rec in recs:
            assert (rec["s64"]["ncontact"] == rec["s32"]["ncontact"]).all() and (rec["s64"]["corner"] == rec["s32"]["corner"]).all(), kind
            assert not rec["left"].any(), kind                             # ... nor for valid cache slots or joints on their stops
    for rec in _free_ref(N):
        assert (rec["s64"]["ncontact"] == rec["s32"]["ncontact"]).all() and (rec["s64"]["corner"] == rec["s32"]["corner"]).all()
    # ... and the fp32 oracle is inside the fixed bound on points and gaps, which its normals are not (module docstring)
    rec = pr.tumbled_teacher_ref("hand_on_box", N)[0]
    sc, _, ms = _setup(N)
    worst_p = max(np.abs(a[:, [0, 1, 2, 6]] - b[:, [0, 1, 2, 6]]).max() for a, b in zip(rec["lists64"], rec["lists32"]) if len(a))
    worst_n = max(np.abs(a[:, 3:6] - b[:, 3:6]).max() for a, b in zip(rec["lists64"], rec["lists32"]) if len(a))
    E = pr.normal_scale(rec["lists64"], rec["lists32"], range(N), sc, ms)
    print(f"\nfp32 oracle against fp64: points / gaps {worst_p:.2e}, normals {worst_n:.2e}, E = {E:.2e} m")
    assert worst_p <= 2e-6 / 10 and 0 < E < 1e-7
    assert min(pr.dist(r, sc, ms) for c in rec["lists64"] for r in c[c[:, 8] == 1]) > 1e-3      # no axis point inside the box: dist is a distance


def test_oracle_gaps_against_independent_capsule_box_distance():
    """Oracle and kernels share one specification of the narrowphase; tests/proximity_ref.seg_box does not.  For every sample-0
    hand / box entry of the fp64 oracle (the axis point nearest to the box: 2^-10 bisection, snapped to an end within 2 %), its
    raw gap D = gap + rest_offset against the exact capsule / box distance Q of that capsule, L its axis length:
    Q <= D + tol and D - Q <= (0.02 + 2^-11) L + tol -- the inequalities and the tol of
    test_proximity.py::test_against_engine_narrowphase, which only meets faces."""
    from tests import proximity_ref as prox
    sc, _, ms = _setup(N)
    hp = prox.HandProx(ms, sc)
    tol = prox.reference(hp, *hp.test_poses(prox.ROWS, prox.SEED))["tol"]["box_d"]
    rec = pr.tumbled_teacher_ref("hand_on_box", N)[0]
    st = rec["start"]
    a, b, _ = hp.capsules(st["q"].T, np.float64)
    box = np.concatenate([st["box_pos"].T, st["box_quat"].T], 1)
    Q = hp.box(a, b, box)[0][..., 0]
    L = np.linalg.norm(b - a, axis=-1)
    R = ts.quat_to_mat(st["box_quat"].T)
    slack, rest = 0.02 + 2.0 ** -11, float(sc.rest_offset)
    valid = rec["wtag64"] == 8 * rec["wgen64"][None, :]
    checked, worst, by_class = 0, [-np.inf, -np.inf], [0, 0, 0]
    for e in range(N):
        c = rec["lists64"][e]
        for cap in np.unique(c[c[:, 8] == 1, 9]).astype(int):
            if not valid[(cap * 2 + 1) * 2, e] or Q[e, cap] <= -hp.r[cap]:   # no sample-0 entry / the axis meets the box
                continue
            row = c[(c[:, 8] == 1) & (c[:, 9] == cap)][0]                    # sample 0 comes first
            D = row[6] + rest
            worst = [max(worst[0], Q[e, cap] - D), max(worst[1], D - Q[e, cap] - slack * L[e, cap])]
            assert Q[e, cap] <= D + tol, (e, cap, Q[e, cap], D)
            assert D - Q[e, cap] <= slack * L[e, cap] + tol, (e, cap, Q[e, cap], D)
            by_class[int((np.abs(R[e].T @ row[3:6]) > 1e-6).sum()) - 1] += 1
            checked += 1
    print(f"\n{checked} sample-0 entries (face, edge, vertex: {by_class}); Q - D <= {worst[0]:.3g}, D - Q - (0.02 + 2^-11) L <= {worst[1]:.3g}, tol {tol:.3g}")
    assert by_class[1] >= 20 and by_class[2] >= 5 and checked >= 100


# ------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False], ids=["k_substep", "k_dynamics+k_solve"])
def test_manifold_on_tumbled_boxes(fused):
    """One sub-step of the hand-on-box sample: the list of every env against the fp64 oracle's (pr.check_manifold).  Measured on one
    MI355X, both launch forms: 885 entries in 256 envs, none left out; E = 3.24e-8 m, worst HIP err_n dist 3.12e-8 m, points and
    gaps within 4.0e-8 m."""
    sc, _, ms = _setup(N)
    rec = pr.tumbled_teacher_ref("hand_on_box", N)[0]
    hb = pr.hip(sc, ms, fused)
    pr.load(hb, rec["start"])
    hb.substep(last=True)
    pr.check_manifold(hb, rec, sc, ms)


# Measured on one MI355X, ratios |HIP - fp64| / |fp32 oracle - fp64| at the 99.9th percentile / at the maximum (the fp32 oracle's own
# figures and the padded runs: DESIGN.md, section 5); C_RULE allows 3:
#              hand on box                       box alone                        free run (test_corner_turnover_free_running)
#              k_substep    k_dynamics+k_solve   k_substep    k_dynamics+k_solve  k_physics4
#   q          0.98 / 0.56  1.00 / 0.57          1.00 / 1.00  1.00 / 1.00
#   qd         0.97 / 0.57  0.97 / 0.58          0.92 / 0.86  1.03 / 0.98
#   box_pos    1.06 / 1.22  1.04 / 1.16          0.92 / 0.85  0.92 / 1.22         1.25 / 1.92
#   box_quat   0.89 / 1.09  0.87 / 1.16          1.00 / 1.12  1.00 / 1.12         1.17 / 1.07
#   box_lin    1.08 / 1.21  1.11 / 1.17          0.81 / 0.78  1.32 / 1.20         0.91 / 1.19
#   box_ang    1.20 / 1.61  1.31 / 1.71          0.95 / 1.00  1.01 / 1.00         0.89 / 0.98
#   cforce     0.87 / 1.20  0.91 / 1.22          0.84 / 0.77  0.86 / 1.19
#   wlam 80-83 1.13 / 1.71  1.16 / 1.80          0.86 / 0.77  1.24 / 1.20         1.40 / 1.62
# (before the stand-alone k_solve took each lane's own contact count in its box-only branch, its box_alone column read 10^4 to 10^5)
@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False], ids=["k_substep", "k_dynamics+k_solve"])
@pytest.mark.parametrize("kind,n", [("hand_on_box", N), ("box_alone", N), ("box_alone", 200)], ids=["hand_on_box", "box_alone", "box_alone-padded"])
def test_teacher_forced_substeps_on_tumbled_boxes(kind, n, fused):
    sc, _, ms = _setup(n)
    pr.check_teacher_forced(lambda: pr.hip(sc, ms, fused), pr.tumbled_teacher_ref(kind, n), kind)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [N, 200], ids=["256", "200-padded"])
def test_corner_turnover_free_running(n):
    """Two physics steps = 8 sub-steps of the tumbling box alone: corners leave the list and move between slots (43 of 256 envs), so
    a slot that kept a stale corner's impulse, or dropped a valid one, shows in the box state."""
    sc, _, ms = _setup(n)
    hb = pr.hip(sc, ms)
    pr.load(hb, pr.tumbled_state("box_alone", n))
    report = {}
    for step, rec in enumerate(_free_ref(n)):
        hb.physics_step()
        sh = pr.snap(hb, pr.BOX_FIELDS)
        pr.check_free_step(sh, rec, f" after step {step}")
        assert sh["ncontact"].max() <= 4
        pr.accumulate_snap(report, rec["s64"], rec["s32"], sh, np.ones(n, bool), pr.BOX_FIELDS)
    pr.assert_c_rule(report, f"free-running, box alone, n = {n}")


@pytest.mark.gpu
def test_hand_on_tumbled_box_is_bitwise_reproducible():
    """test_general_contact_path_is_bitwise_reproducible on the hand-on-box sample: two instances, two physics steps."""
    import torch
    sc, _, ms = _setup(N)
    outs = []
    for _ in range(2):
        hb = pr.hip(sc, ms)
        pr.load(hb, pr.tumbled_state("hand_on_box", N))
        hb.physics_step(), hb.physics_step()
        torch.cuda.synchronize()
        outs.append([hb.core.field(f).clone() for f in pr.SYNC + ("cforce", "wlam", "wgen", "ncontact")])
    assert outs[0][-1].max() > 4
    for a, b in zip(*outs):
        assert torch.equal(a, b)
