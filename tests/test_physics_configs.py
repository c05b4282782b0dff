"""The physics kernels at NON-DEFAULT physics and box configurations, against the fp64 and fp32 oracles: the method of
tests/test_tumbled_box.py (teacher-forced sub-steps on tumbled boxes, bounds from the fp32 oracle's own error) along the configuration
axis.  Every other GPU physics test runs one contact_offset / rest_offset / max_depenetration_velocity, one box size, one ground and hand
friction, one dt, one erp and a gravity along z; a literal left in a kernel for any of them would pass the suite.

Configurations (CONFIGS): each goes through default_cfg("BlindGrasping") and build_sim_config; ground_friction (hard-wired in config.py)
and hand_friction (fixed by the MJCF-less model) are set on the built DexSimConfig / HandModel before to_struct().
  fast_yaml   the reference's cfg/physics/fast.yaml in full
  big_box     0.08 m, 0.25 kg, box friction 0.6, placed at z = 0.13; ground friction 0.9, hand friction 0.7
  small_box   0.03 m, 0.04 kg, box friction 0.6, placed at z = 0.13; the same two frictions
  world       dt at 0.8 x the task's, gravity (0.8, -0.5, -9.2), erp 0.35, max_depenetration_velocity 0.02
Two settings are further from the default than a first guess would put them, because the field must bite (below).  The boxes are placed
0.09 and 0.115 m above their rest height (0.04, 0.015): the control steps see the box only through the rewards (no policy observation
holds it), whose box terms at rest heights differ from the default placement by 4-9 bounds, at 0.13 by 17.  fast.yaml's
max_depenetration_velocity = 0.5 cannot bite on these samples: the cap acts on erp |gap| / h, which stays below the default 0.2 m/s as
well (test_fast_yaml_depenetration_cap_is_out_of_reach), so `world` carries a cap of 0.02 m/s, which does.

Samples: tests/tumbled_states.py drawn per configuration, N = 256, seed 11 (four workgroups, every box class in each); the GPU tests
also run the first 200 envs (last workgroup padded).  "hand_on_box" has the hand 0-2 mm past its first touch, "hand_near_box" 2-4 mm
short of it: capsules fail their broadphase bounds while nothing of the hand touches, so hand_clear and capsule_clear are met on both
sides of their decision at a 2 mm contact offset and at both box sizes.

Bounds: none of this file's own.  Integers exact over the envs whose list length agrees in both oracles and the kernels, at most
LEFT_OUT = 2 % left out; points and gaps 2e-6 m; normals c E / dist + 1e-7; states c x the fp32 oracle's own error at the 99.9th
percentile and at the maximum plus the floors 1e-7 and 1e-6, c = 3: all through the functions of tests/physics_rig.py, which has
them from test_gpu_parity.py::test_hip_error_is_a_small_multiple_of_fp32_roundoff.  Whole control steps: the assertions of
test_gpu_parity.py::test_other_substep_counts_match_oracle.  Queries: 4 x the fp32 reference's own error, through the functions those
suites share (tests/kindyn_ref.py, tests/invdyn_ref.py, tests/proximity_ref.py).

The CPU tests show that the references alone meet what the GPU tests rely on (both oracles list the same contacts, nothing left out),
and that every varied field BITES: the fp64 oracle with that one field back at its default differs from the configured one by at least
10 x the bound in a quantity a GPU test compares, and an fp32 oracle so built, put in the kernels' place through the same comparison
functions, misses the bound.  A kernel that ignored the field would therefore fail.  Measured figures: DESIGN.md, section 5.
"""
import functools

import numpy as np
import pytest

from dexrobot_isaac_amd.config import default_cfg
from tests import physics_rig as pr
from tests import tumbled_states as ts

N, PADDED = pr.N, 200
N_STEP = 130                            # whole control steps: test_other_substep_counts_match_oracle's size
N_QUERY = 70                            # the query suites' size
BITE = 10.0                             # a field put back must move a compared quantity by this many bounds (a condition on the input)

_DT = default_cfg("BlindGrasping")["sim"]["dt"]
CONFIGS = {
    "fast_yaml": {"sim.substeps": 2, "sim.physx.num_position_iterations": 8, "sim.physx.contact_offset": 0.002,
                  "sim.physx.rest_offset": 0.001, "sim.physx.max_depenetration_velocity": 0.5},
    "big_box": {"env.box.size": 0.08, "env.box.mass": 0.25, "env.box.friction": 0.6, "env.box.initial_position.z": 0.13,
                "ground_friction": 0.9, "hand_friction": 0.7},
    "small_box": {"env.box.size": 0.03, "env.box.mass": 0.04, "env.box.friction": 0.6, "env.box.initial_position.z": 0.13,
                  "ground_friction": 0.9, "hand_friction": 0.7},
    "world": {"sim.dt": 0.8 * _DT, "sim.gravity.0": 0.8, "sim.gravity.1": -0.5, "sim.gravity.2": -9.2, "sim.dexsim_erp": 0.35,
              "sim.physx.max_depenetration_velocity": 0.02},
}
SEEDS = {name: pr.SEED for name in CONFIGS}          # a configuration whose sample conditions fail gets another seed, not another condition
NAMES = list(CONFIGS)
CAP = "sim.physx.max_depenetration_velocity"
PAIRS = [(name, field) for name in NAMES for field in CONFIGS[name] if (name, field) != ("fast_yaml", CAP)]
KINDS = ("hand_on_box", "box_alone", "hand_near_box")


def _fields(name, back=None):
    """Configuration `name` as the keywords of pr.setup; `back`: one of its fields left at the default."""
    return {k: v for k, v in CONFIGS[name].items() if k != back}


def _setup(name, n, back=None, episode_length=None):
    """(sc, model, ms) of configuration `name` for n envs."""
    more = {} if episode_length is None else {"env.episodeLength": episode_length}
    return pr.setup("BlindGrasping", n, **more, **_fields(name, back))


def _state(name, kind, n):
    """The first n envs of the configuration's N-env sample (always drawn for the configuration itself, never for a `back` variant)."""
    return pr.tumbled_state(kind, n, SEEDS[name], **_fields(name))


def _teacher_ref(name, kind, n):
    return pr.tumbled_teacher_ref(kind, n, SEEDS[name], **_fields(name))


def _physics_ref(name, kind, n):
    """One physics step (sim.substeps sub-steps, free-running) of the sample on both oracles."""
    return pr.tumbled_free_ref(kind, n, 1, pr.FIELDS, SEEDS[name], **_fields(name))[0]


def _hand_entries(lists):
    return int(sum((c[:, 8] != 2).sum() for c in lists))


# ------------------------------------------------------------------------------------------------- the comparisons (GPU tests and stand-ins)
def _check_lists(make, name):
    """3.1: the first teacher-forced sub-step of hand_on_box, pr.check_manifold."""
    sc, _, ms = _setup(name, N)
    rec = _teacher_ref(name, "hand_on_box", N)[0]
    b = make()
    pr.load(b, rec["start"])
    b.substep(last=True)
    pr.check_manifold(b, rec, sc, ms)


def _check_teacher(make, name, kind, n):
    return pr.check_teacher_forced(make, _teacher_ref(name, kind, n), kind, label=f"{name}, ")


def _check_physics_step(make, name, kind, n):
    """One free-running physics step: contact counts and slot corners exact against both oracles, states by the c rule.  On
    hand_near_box also the first sub-step alone: no hand entry in any env, the lists of pr.check_manifold's kind."""
    b = make()
    if kind == "hand_near_box":
        rec = _teacher_ref(name, kind, n)[0]
        pr.load(b, rec["start"])
        b.substep(last=True)
        lists = pr.lists(b, n)
        assert _hand_entries(lists) == 0 and _hand_entries(rec["lists64"]) == 0, "a hand entry where nothing of the hand touches"
        assert all(pr.same_lists(a, c) for a, c in zip(rec["lists64"], lists))
        assert (pr.bg_cache(b)[1] == rec["s64"]["corner"]).all()
        b = make()
    ref = _physics_ref(name, kind, n)
    pr.load(b, _state(name, kind, n))
    b.physics_step()
    sh = pr.snap(b)
    pr.check_free_step(sh, ref)
    report = {}
    pr.accumulate_snap(report, ref["s64"], ref["s32"], sh, np.ones(n, bool), pr.FIELDS)
    pr.assert_c_rule(report, f"one physics step, {name}, {kind}, n = {n}")
    return report


def _check_control_steps(o, hb):
    """12 random-action control steps with in-step resets (env.episodeLength = 8) of `hb` against the fp32 oracle `o`, at the bars of
    test_gpu_parity.py::test_other_substep_counts_match_oracle."""
    pr.control_steps(o, hb, np.random.default_rng(13), 12, reset_atol=2e-4, obs_bar=5e-3, rew_atol=2e-2, rew_rtol=1e-4, q_atol=5e-4)


# ------------------------------------------------------------------------------------------------- CPU: the samples
@pytest.mark.parametrize("name", NAMES)
def test_sample_conditions(name):
    """Per configuration and kind: both oracles list the same contacts (length, type, capsule, corner per slot) in every env after
    each of three teacher-forced sub-steps and after the free physics step -- none is left out; hand_on_box: every env has a hand
    entry, hand / ground and hand / box entries both occur; hand_near_box: no hand entry in any env, in either oracle."""
    sc, _, ms = _setup(name, N)
    for kind in KINDS:
        recs = _teacher_ref(name, kind, N)
        assert all(pr.same_lists(a, b) for a, b in zip(recs[0]["lists64"], recs[0]["lists32"])), kind
        for rec in recs:
            assert (rec["s64"]["ncontact"] == rec["s32"]["ncontact"]).all() and (rec["s64"]["corner"] == rec["s32"]["corner"]).all(), kind
            assert not rec["left"].any(), kind                             # (pr.oracles_differ: valid cache slots and joint stops too)
        if kind != "hand_on_box":
            ref = _physics_ref(name, kind, N)
            assert (ref["s64"]["ncontact"] == ref["s32"]["ncontact"]).all() and (ref["s64"]["corner"] == ref["s32"]["corner"]).all(), kind
    on = _teacher_ref(name, "hand_on_box", N)[0]
    types = np.concatenate([c[:, 8] for c in on["lists64"]]).astype(int)
    assert all((c[:, 8] != 2).any() for c in on["lists64"])
    hand_ground, hand_box = int((types == 0).sum()), int((types == 1).sum())
    near = _teacher_ref(name, "hand_near_box", N)[0]
    E = pr.normal_scale(on["lists64"], on["lists32"], range(N), sc, ms)
    print(f"\n{name}: hand / ground {hand_ground}, hand / box {hand_box} entries; E = {E:.3e} m; box / ground counts 0-4 (box alone): "
          f"{np.bincount(_teacher_ref(name, 'box_alone', N)[0]['s64']['ncontact'], minlength=5).tolist()}")
    assert hand_ground > 0 and hand_box > 0
    assert _hand_entries(near["lists64"]) == 0 and _hand_entries(near["lists32"]) == 0
    assert max(c.shape[0] for c in near["lists64"]) <= 4
    # ... and the near hand is within 4 mm of touching: with the slide that much further down (at or below the ladder's first touching
    # rung) every env has a hand entry
    from oracle.oracle import Oracle
    lower = Oracle(sc, ms, f64=True)
    st = _state(name, "hand_near_box", N)
    st["q"][2] = ts.f32(st["q"][2] - 0.004)
    pr.load(lower, st)
    lower.substep(last=True)
    assert all((c[:, 8] != 2).any() for c in pr.lists(lower, N))
    assert 0 < E < 1e-7 and min(pr.dist(r, sc, ms) for c in on["lists64"] for r in c[c[:, 8] == 1]) > 1e-3


# ------------------------------------------------------------------------------------------------- CPU: each varied field bites
def _margins_substep(name, back):
    """The fp64 oracle with `back` at its default against the configured one, first teacher-forced sub-step of hand_on_box: for every
    quantity the GPU tests compare, the difference in units of the bound they apply to it."""
    from oracle.oracle import Oracle
    rec = _teacher_ref(name, "hand_on_box", N)[0]
    sc, _, ms = _setup(name, N, back)
    o = Oracle(sc, ms, f64=True)
    pr.load(o, rec["start"])
    o.substep(last=True)
    s, lists = pr.snap(o), pr.lists(o, N)
    m = {}
    same = s["ncontact"] == rec["s64"]["ncontact"]
    m["list length"] = (1.0 - same.mean()) / pr.LEFT_OUT                      # the bound on envs whose lists differ in length
    if not same.any():
        return m
    gaps = [np.abs(a[:, [0, 1, 2, 6, 7]] - b[:, [0, 1, 2, 6, 7]]).max() for a, b in zip(lists, rec["lists64"]) if a.shape == b.shape and len(a)]
    m["points / gaps / mu"] = max(gaps, default=0.0) / 2e-6
    for f in pr.FIELDS:
        e32 = np.abs(rec["s32"][f] - rec["s64"][f])[:, same].max()
        m[f] = np.abs(s[f] - rec["s64"][f])[:, same].max() / (pr.C_RULE * e32 + 1e-6)
    ok = np.repeat((s["corner"] >= 0) & (s["corner"] == rec["s64"]["corner"]) & (rec["s32"]["corner"] == rec["s64"]["corner"]) & same, 3, axis=0)
    if ok.any():
        m["wlam 80-83"] = np.abs(s["lam"] - rec["s64"]["lam"])[ok].max() / (pr.C_RULE * np.abs(rec["s32"]["lam"] - rec["s64"]["lam"])[ok].max() + 1e-6)
    return m


@functools.lru_cache(maxsize=None)
def _control_ref(name, back=None):
    """reset + one control step (zero actions) of the fp64 oracle: observations, rewards, q."""
    from oracle.oracle import Oracle
    sc, _, ms = _setup(name, N_STEP, back, 8)
    o = Oracle(sc, ms, f64=True)
    obs0 = o.reset().astype(np.float64)
    obs, rew, _ = o.step(np.zeros((N_STEP, 18), np.float32))
    return dict(obs0=obs0, obs=obs.astype(np.float64), rew=rew.astype(np.float64), q=o.get("q"))


def _margins_control(name, back):
    a, b = _control_ref(name, back), _control_ref(name)
    return {"reset obs": np.abs(a["obs0"] - b["obs0"]).max() / 2e-4, "obs": np.abs(a["obs"] - b["obs"]).max() / 5e-3,
            "rew": (np.abs(a["rew"] - b["rew"]) / (2e-2 + 1e-4 * np.abs(b["rew"]))).max(), "final q": np.abs(a["q"] - b["q"]).max() / 5e-4}


@pytest.mark.parametrize("name,field", PAIRS, ids=[f"{n}-{f}" for n, f in PAIRS])
def test_each_varied_field_bites(name, field):
    """A kernel that ignored `field` (took its default) would fail a GPU test of this file: (1) the fp64 oracle so built moves a
    compared quantity by at least BITE = 10 bounds -- one sub-step of hand_on_box for the teacher-forced quantities, reset + one control
    step for the box placement and the L2 uses of box_size; (2) the fp32 oracle so built, in the kernels' place, is refused by the
    very comparison functions the GPU tests call."""
    from oracle.oracle import Oracle
    m = dict(_margins_substep(name, field))
    m.update(_margins_control(name, field))
    print(f"\n{name}, {field} at its default: difference / bound = " + ", ".join(f"{k} {v:.3g}" for k, v in m.items()))
    assert max(m.values()) >= BITE, (name, field, m)

    def stand_in(n, episode_length=None):
        sc, _, ms = _setup(name, n, field, episode_length)
        return Oracle(sc, ms)

    checks = (lambda: _check_lists(lambda: stand_in(N), name),
              lambda: _check_teacher(lambda: stand_in(N), name, "hand_on_box", N),
              lambda: _check_teacher(lambda: stand_in(N), name, "box_alone", N),
              lambda: _check_control_steps(Oracle(*_setup(name, N_STEP, None, 8)[::2]), stand_in(N_STEP, 8)))
    for check in checks:
        try:
            check()
        except AssertionError:
            return
    pytest.fail(f"{name}: an fp32 oracle with {field} at its default passes every comparison")


def test_fast_yaml_depenetration_cap_is_out_of_reach():
    """Why (fast_yaml, max_depenetration_velocity) is not among the pairs above: the cap acts on erp |gap| / h of a penetrating entry,
    and on the fast_yaml samples that stays below the default cap of 0.2 m/s, hence below fast.yaml's 0.5 as well -- the two builds
    compute the same thing, to the bit, with the hand 0-2 mm past its first touch.  `world` varies the field where it acts."""
    from oracle.oracle import Oracle
    sc, _, _ = _setup("fast_yaml", N)
    default = default_cfg("BlindGrasping")["sim"]["physx"]["max_depenetration_velocity"]
    h = float(sc.dt) / int(sc.substeps)
    for kind in ("hand_on_box", "box_alone"):
        rec = _teacher_ref("fast_yaml", kind, N)[0]
        deepest = min(c[:, 6].min() for c in rec["lists64"] if len(c))
        assert 0 < -deepest * float(sc.erp) / h < default < float(sc.max_depenetration_velocity), (kind, deepest)
    back = Oracle(*_setup("fast_yaml", N, CAP)[::2], f64=True)
    pr.load(back, rec["start"])
    back.substep(last=True)
    assert all(np.array_equal(back.get(f), rec["s64"][f]) for f in pr.FIELDS)


def test_stand_in_of_the_configuration_itself_passes():
    """The other half of the stand-in argument: an fp32 oracle built from the configuration itself passes the same comparisons."""
    from oracle.oracle import Oracle
    for name in NAMES:
        make = lambda: Oracle(*_setup(name, N)[::2])
        _check_lists(make, name)
        _check_teacher(make, name, "hand_on_box", N)
        for kind in ("box_alone", "hand_near_box"):
            _check_physics_step(make, name, kind, N)


# ------------------------------------------------------------------------------------------------- CPU: the queries' conditions
@functools.lru_cache(maxsize=None)
def _world_gravity_ref():
    from tests import kindyn_ref as kr
    sc, _, ms = _setup("world", N_QUERY)
    q = kr.HandKin(ms).random_poses(N_QUERY, 21)
    o32, o64 = kr.oracle_pair(sc, ms)
    M32, g32 = kr.mass_gravity(o32, q)
    M64, g64 = kr.mass_gravity(o64, q)
    return dict(q=q, M64=M64, g64=g64, e_M=kr.err_M(M32, M64), e_g=kr.err_g(g32, g64, M64))


def test_world_gravity_loads_the_x_and_y_slides():
    """In the fp64 reference the gravity force on the x and y slides is at least 1 % of that on the z slide for every pose, and a
    reference that ignored g.x or g.y misses the 4 e_g bound of test_kindyn.py by BITE."""
    from tests import kindyn_ref as kr
    r = _world_gravity_ref()
    g = r["g64"]
    assert (np.abs(g[:, 0]) >= 0.01 * np.abs(g[:, 2])).all() and (np.abs(g[:, 1]) >= 0.01 * np.abs(g[:, 2])).all()
    for back in ("sim.gravity.0", "sim.gravity.1", "sim.gravity.2"):
        sc, _, ms = _setup("world", N_QUERY, back)
        _, galt = kr.mass_gravity(kr.oracle_pair(sc, ms)[1], r["q"])
        assert kr.err_g(galt, g, r["M64"]) >= BITE * 4 * r["e_g"], back


@functools.lru_cache(maxsize=None)
def _big_box_proximity_ref():
    from tests import proximity_ref as prox
    sc, _, ms = _setup("big_box", N_QUERY)
    hp = prox.HandProx(ms, sc)
    q, box = hp.test_poses(N_QUERY, prox.SEED)
    return dict(prox.reference(hp, q, box), hp=hp, q=q, box=box)


def test_big_box_proximity_reference_differs_from_the_default_size():
    r = _big_box_proximity_ref()
    assert r["hp"].box_size == pytest.approx(0.08)
    other = r["hp"].query(r["q"], r["box"], 0.05)
    d = np.abs(other["cap_env"][:, :, 0, 0] - r["r64"]["cap_env"][:, :, 0, 0])[r["sel"]["box_d"]].max()
    assert d >= BITE * r["tol"]["box_d"]


# ------------------------------------------------------------------------------------------------- GPU
def _hip(name, n, fused=True, episode_length=None):
    sc, _, ms = _setup(name, n, None, episode_length)
    return pr.hip(sc, ms, fused)


FORMS = pytest.mark.parametrize("fused", [True, False], ids=["k_substep", "k_dynamics+k_solve"])


@pytest.mark.gpu
@FORMS
@pytest.mark.parametrize("name", NAMES)
def test_contact_lists(name, fused):
    _check_lists(lambda: _hip(name, N, fused), name)


@pytest.mark.gpu
@FORMS
@pytest.mark.parametrize("kind,n", [("hand_on_box", N), ("hand_on_box", PADDED), ("box_alone", N), ("box_alone", PADDED)],
                         ids=["hand_on_box", "hand_on_box-padded", "box_alone", "box_alone-padded"])
@pytest.mark.parametrize("name", NAMES)
def test_teacher_forced_substeps(name, kind, n, fused):
    """Measured ratios: DESIGN.md, section 5."""
    _check_teacher(lambda: _hip(name, n, fused), name, kind, n)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["box_alone", "hand_near_box"])
@pytest.mark.parametrize("name", NAMES)
def test_one_fused_physics_step(name, kind):
    """fast_yaml: two single-sub-step launches; the others: one k_physics4 launch."""
    _check_physics_step(lambda: _hip(name, N), name, kind, N)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_fused_physics_launch_equals_single_substep_launches(name):
    """test_gpu_parity.py::test_fused_physics_launch_equals_four_single_substep_launches on hand_on_box, per configuration: the state
    after one sim.dt is bit-identical to that after sim.substeps single sub-step launches."""
    import torch
    from dexrobot_isaac_amd import _abi
    a, b = _hip(name, N), _hip(name, N)
    st = _state(name, "hand_on_box", N)
    pr.load(a, st), pr.load(b, st)
    a.core.run_stage(_abi.STAGE["PHYSICS"])
    for _ in range(int(_setup(name, N)[0].substeps)):
        b.core.run_stage(_abi.STAGE["SUBSTEP"])
    torch.cuda.synchronize()
    assert a.get("ncontact").max() > 4
    for f in ("q", "qd", "box_pos", "box_quat", "box_lin", "box_ang", "site_pose", "ncontact", "cforce"):
        assert np.array_equal(a.get(f), b.get(f)), f


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_control_steps_with_resets(name):
    """Whole control steps with in-step resets: the reset's box placement at the configured box_z, the L2 block's box_size terms;
    fast_yaml is the true physics=fast case."""
    from oracle.oracle import Oracle
    sc, _, ms = _setup(name, N_STEP, None, 8)
    _check_control_steps(Oracle(sc, ms), _hip(name, N_STEP, episode_length=8))


@pytest.mark.gpu
def test_queries_under_world_gravity():
    """dexsim_mass_matrix's gravity force and dexsim_inverse_dynamics with DEXSIM_ID_GRAVITY against the fp64 oracle built from the
    `world` configuration: 4 x the fp32 oracle's own error (test_kindyn.py, test_inverse_dynamics.py)."""
    from dexrobot_isaac_amd.core import DexSimCore
    from tests import invdyn_ref as ir
    from tests import kindyn_ref as kr
    from tests.query_rig import pose_core
    sc, _, ms = _setup("world", N_QUERY)
    r = _world_gravity_ref()
    core = DexSimCore(sc, ms, "cuda:0")
    core.reset()
    qd, qdd = ir.random_rates(N_QUERY, 31)
    pose_core(core, r["q"], qd=qd)
    M, g = kr.gpu_mass(core, N_QUERY)
    E_M, E_g = kr.err_M(M, r["M64"]), kr.err_g(g, r["g64"], r["M64"])
    print(f"\nworld: E_M = {E_M:.3g} (fp32 oracle {r['e_M']:.3g}), E_g = {E_g:.3g} (fp32 oracle {r['e_g']:.3g})")
    assert not np.isnan(M).any() and not np.isnan(g).any()
    assert E_M <= 4 * r["e_M"] and E_g <= 4 * r["e_g"]
    o32, o64 = kr.oracle_pair(sc, ms)
    M64, b64 = ir.mass_bias(o64, r["q"], qd)
    M32, b32 = ir.mass_bias(o32, r["q"], qd)
    full64 = ir.tau_of(M64, b64, qdd)
    e_full = ir.err_tau(ir.tau_of(M32, b32, qdd, np.float32), full64, M64)
    e_bias = ir.err_tau(b32.astype(np.float32), b64, M64)
    ir.check_tau(ir.gpu_tau(core, N_QUERY, qdd=qdd), full64, M64, e_full, "world, full (qdd, gravity)")
    ir.check_tau(ir.gpu_tau(core, N_QUERY), b64, M64, e_bias, "world, bias force (gravity)")
    ir.check_tau(ir.gpu_tau(core, N_QUERY, q=r["q"], qd=np.zeros_like(qd)), r["g64"], r["M64"], r["e_g"], "world, gravity force alone")


@pytest.mark.gpu
def test_proximity_takes_the_configured_box_size():
    """dexsim_query_proximity with box_size = 0 under big_box against tests/proximity_ref.py at 0.08, test_proximity.py's bounds."""
    from dexrobot_isaac_amd.core import DexSimCore
    from tests import proximity_ref as prox
    from tests.query_rig import pose_core
    sc, _, ms = _setup("big_box", N_QUERY)
    r = _big_box_proximity_ref()
    core = DexSimCore(sc, ms, "cuda:0")
    core.reset()
    pose_core(core, r["q"], r["box"])
    prox.check_against(prox.gpu_query(core, N_QUERY), r, label="big_box, box_size = 0: ")
