"""GPU parity tests (-m gpu): the HIP kernels, called through the C-ABI, against
  (1) the golden vectors produced by the reference's own Python (L2), and
  (2) the CPU oracle on identical seeded state (physics; teacher-forced sub-steps and free-running steps).
Tolerances are stated per test; integer / boolean outputs must match exactly.  Configurations, the loaded backends and the
comparisons that more than one test uses: tests/physics_rig.py."""
import os

import numpy as np
import pytest

from dexrobot_isaac_amd.config import build_sim_config, default_cfg
from tests import physics_rig as pr
from tests.l2_replay import ALL_SCENARIOS as SCENARIOS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", SCENARIOS)
def test_hip_l2_replays_reference_golden(golden_dir, name):
    from tests.l2_replay import replay, scenario_config
    npz = np.load(os.path.join(golden_dir, f"l2_{name}.npz"), allow_pickle=False)
    sc, model = build_sim_config(scenario_config(npz))
    hb = pr.hip(sc, model.to_struct())
    err = replay(hb, npz)     # obs within 2e-5 abs / 1e-5 rel, rewards 2e-6 rel, done exact
    assert err["obs"] < 2e-5 and err["active_prev_targets"] < 1e-6
    # the replay also compared, ON THE HIP PATH: every final obs_dict component and reward component of the scenario, the
    # per-step success / failure / timeout rates and consecutive successes, and in the round-2 scenarios (N = 70: two
    # workgroups, one of them padded; default-length FSM) the explicit reset_idx(ids) events and per-step snapshots of every
    # obs_dict key and every reward component
    assert any(k.startswith("final:") for k in err) and any(k.startswith("final_rc:") for k in err) and "stats" in err
    if name in ("blind_wide", "base_wide"):
        assert any(k.startswith("ev:") for k in err) and any(k.startswith("snap:") for k in err) and any(k.startswith("snap_rc:") for k in err)
    if "_cfg_" in name:       # non-default configurations: snapshots, every criterion's raw condition, the binary observations
        assert any(k.startswith("snap:") for k in err) and any(k.startswith("snap_rc:") for k in err)
        assert err["crit_fail"] == 0 and err["crit_succ"] == 0 and err["binaries"] == 0
        assert ("ev:targets" in err) == (name in ("blind_cfg_base", "base_cfg_base"))


@pytest.mark.parametrize("fused", [True, False], ids=["k_substep", "k_dynamics+k_solve"])
@pytest.mark.parametrize("task", ["BlindGrasping", "BaseTask"])
def test_teacher_forced_substep_matches_oracle(task, fused):
    """One sub-step (dynamics + contact solve + integrate) from identical state.
    Tolerance: 2e-4 abs on q / box pose, 2e-3 on velocities (PGS amplifies fp32 roundoff of the two
    factorisations: dense Cholesky in the oracle vs Schur-complement blocks on the GPU), contact count exact."""
    n = 256
    sc, model, ms = pr.setup(task, n)
    st = pr.random_state(np.random.default_rng(5), model, n)
    o, hb = pr.backends(sc, ms, {k: v for k, v in st.items() if task == "BlindGrasping" or not k.startswith("box")}, fused=fused)
    for sub in range(3):
        o.substep(last=True)
        hb.substep(last=True)
        nc_o, nc_h = o.get("ncontact")[0], hb.get("ncontact")[0]
        assert (nc_o == nc_h).all(), f"contact count differs in {(nc_o != nc_h).sum()} envs at sub-step {sub}"
        np.testing.assert_allclose(hb.get("q"), o.get("q"), atol=2e-4)
        np.testing.assert_allclose(hb.get("qd"), o.get("qd"), atol=5e-3, rtol=2e-3)
        np.testing.assert_allclose(hb.get("cforce"), o.get("cforce"), atol=5e-2, rtol=2e-2)
        if task == "BlindGrasping":
            np.testing.assert_allclose(hb.get("box_pos"), o.get("box_pos"), atol=2e-4)
            np.testing.assert_allclose(hb.get("box_lin"), o.get("box_lin"), atol=5e-3, rtol=2e-3)
        # re-synchronise (teacher forcing) so that each sub-step is compared from identical state
        for k in ("q", "qd", "box_pos", "box_quat", "box_lin", "box_ang"):
            if task == "BaseTask" and k.startswith("box"):
                continue
            hb.set(k, o.get(k))
    assert o.get("ncontact").max() >= 5          # the sample really contains finger/box and ground contacts
    o.publish()
    hb.publish()
    np.testing.assert_allclose(hb.get("site_pose"), o.get("site_pose"), atol=2e-6)
    np.testing.assert_allclose(hb.get("hand_vel"), o.get("hand_vel"), atol=2e-5)


@pytest.mark.parametrize("z_range", [(-0.1, 0.2), (-0.36, -0.30), (-0.43, -0.38), (-0.222, -0.216)],
                         ids=["hand_clear", "sphere_fails_capsules_clear", "touching", "capsules_near_nothing_touches"])
def test_broadphase_regimes_match_oracle(z_range):
    """The sub-step kernel has three regimes per workgroup -- hand bounding sphere clear (early box solve), sphere not
    clear but every capsule passes its bounds, and the general contact path -- and mixes of them across workgroups.
    Each must give the oracle's contact lists and state after a full physics step (4 sub-steps in one launch)."""
    n = 320                                          # 5 workgroups
    sc, model, ms = pr.setup("BlindGrasping", n)
    rng = np.random.default_rng(17)
    st = pr.random_state(rng, model, n)
    st["q"][2] = rng.uniform(z_range[0], z_range[1], n)
    if z_range == (-0.222, -0.216):                  # straight fingers a few mm to 3 cm off the box: capsule bounds fail, nothing touches (the box-only fast-out)
        st["q"][:2] = rng.uniform(-0.01, 0.01, (2, n)); st["q"][3:6] = 0.0; st["q"][6:] = rng.uniform(0.0, 0.05, (20, n))
        st["qd"] *= 0.1
        st["box_pos"][:2] *= 0.3
        st["q"][2, 64:128] = rng.uniform(-0.43, -0.38, 64)     # ... and one workgroup that does touch
        # ... and two workgroups in which NO env can touch although the middle finger's capsules fail their bounds: hand centred over
        # the box, fingertips 2-14 mm above its top face
        st["q"][:2, 192:] = 0.0; st["q"][2, 192:] = rng.uniform(-0.238, -0.226, 128)
        st["box_pos"][:2, 192:] = 0.0; st["box_quat"][:, 192:] = np.array([[0.0], [0.0], [0.0], [1.0]])
        st["box_lin"][:, 192:] = 0.0; st["box_ang"][:, 192:] = 0.0; st["qd"][:, 192:] = 0.0
    st["q"][2, :64] = rng.uniform(-0.1, 0.2, 64)    # first workgroup always far from the box: regimes mix across workgroups
    st["q"] = np.clip(st["q"], model.lo[:, None] + 1e-3, model.hi[:, None] - 1e-3)
    st["targets"] = st["q"] + rng.normal(0, 0.02, (26, n))
    st["qd"] *= 0.2
    if z_range == (-0.222, -0.216):
        st["targets"][:, 192:] = st["q"][:, 192:]    # (the hands of the contact-free workgroups hold their pose)
    o, hb = pr.backends(sc, ms, st)
    o.physics_step()
    hb.physics_step()
    nc_o, nc_h = o.get("ncontact")[0], hb.get("ncontact")[0]
    assert (nc_o == nc_h).all(), f"contact count differs in {(nc_o != nc_h).sum()} envs"
    if z_range[0] > -0.2:
        assert nc_o.max() <= 4                       # box/ground contacts only
    if z_range[1] < -0.37:
        assert nc_o.max() >= 5                       # fingers really touch box or ground
    if z_range == (-0.222, -0.216):
        assert nc_o[192:].max() <= 4 and nc_o[64:128].max() >= 5
    np.testing.assert_allclose(hb.get("q"), o.get("q"), atol=5e-4)
    np.testing.assert_allclose(hb.get("box_pos"), o.get("box_pos"), atol=5e-4)
    np.testing.assert_allclose(hb.get("box_lin"), o.get("box_lin"), atol=2e-2, rtol=5e-3)
    np.testing.assert_allclose(hb.get("site_pose"), o.get("site_pose"), atol=5e-4)


def test_split_schur_phase_matches_the_one_wave_version():
    """Hand clear of box and ground in every workgroup: the fused sub-step splits the Schur phase over four waves (three
    helpers post their shares of S, the bias and the G^T tau sum through LDS behind tokens) while the staged k_dynamics
    runs it on one wave.  Same expressions, same accumulation order -- the two launches still differ in where the compiler
    contracts multiply-adds, so the comparison is to a few ulp (2e-6 of the largest velocity, 1e-7 on positions), which a
    wrong or stale hand-over word would miss by orders of magnitude; padded lanes included."""
    n = 200                                          # 4 workgroups, the last one padded
    sc, model, ms = pr.setup("BlindGrasping", n)
    a, b = pr.hip(sc, ms, fused=True), pr.hip(sc, ms, fused=False)
    rng = np.random.default_rng(23)
    st = pr.random_state(rng, model, n, near_box=False)
    st["q"][2] = rng.uniform(-0.05, 0.2, n)
    st["q"] = np.clip(st["q"], model.lo[:, None] + 1e-3, model.hi[:, None] - 1e-3)
    pr.load(a, st), pr.load(b, st)
    for sub in range(3):
        a.substep(last=True)
        b.substep(last=True)
        assert a.get("ncontact").max() <= 4          # box/ground contacts only: the split path ran
        x, y = a.get("qd"), b.get("qd")
        assert np.abs(x - y).max() <= 2e-6 * max(1.0, np.abs(y).max()), f"qd differs after sub-step {sub}: {np.abs(x - y).max():.3e}"
        np.testing.assert_allclose(a.get("q"), b.get("q"), atol=1e-7, rtol=0)
        for k in ("q", "qd"):                        # both continue from the same state: no drift accumulates in the comparison
            a.set(k, b.get(k))


def test_contact_manifold_matches_oracle():
    """Narrowphase only: identical contact lists (type, capsule, order) and geometry within 1e-6."""
    n = 128
    sc, model, ms = pr.setup("BlindGrasping", n)
    o, hb = pr.backends(sc, ms, pr.random_state(np.random.default_rng(9), model, n))
    o.substep(last=True)
    hb.substep(last=True)
    total = 0
    for e in range(n):
        co = o.contacts(e)
        pr.assert_same_entries(co, hb.contacts(e), atol=2e-6)
        total += len(co)
    assert total > 4 * n


def test_free_running_steps_match_oracle():
    """Whole env.step() pipeline for 30 control steps with the same device/host Philox reset stream.
    fp32 roundoff grows through contacts, so the bar is statistical for trajectories (median obs error
    < 1e-4, 99th percentile < 5e-3) and exact for the integer bookkeeping of envs that did not diverge."""
    n = 192
    sc, _, ms = pr.setup("BlindGrasping", n, **{"env.episodeLength": 25})      # (timeouts at 24)
    o, hb = pr.backends(sc, ms)
    pr.free_running(o, hb, np.random.default_rng(3), 30, reset_atol=2e-4, median=1e-4, p99=5e-3, mismatches=2, resets=2)
    # the contact solver's warm-start cache went through the same life on both sides: one generation per sub-step and reset,
    # the same slots valid (tag = 8 * generation [+ corner]), the same impulses in them
    lam_h, tag_h, gen_h = hb.warm_cache()
    lam_o, tag_o, gen_o = o.warm_cache()
    assert (gen_h == gen_o).all() and gen_o.min() >= 30 * 4
    valid_o, valid_h = (tag_o >> 3) == gen_o, (tag_h >> 3) == gen_h
    agree = (valid_o == valid_h).all(axis=0)
    assert agree.mean() > 0.97                               # (an env whose contact set differs has diverged: counted above)
    sel = np.repeat(valid_o & valid_h, 3, axis=0) & agree
    assert sel.sum() > 3 * 4 * n // 2                        # the resting boxes' ground contacts, at least
    assert np.percentile(np.abs(lam_h - lam_o)[sel], 99) < 1e-4


def test_body_states_and_indexed_setters():
    import torch
    n = 70                                                   # not a multiple of 64: padded lanes exercised
    sc, model, ms = pr.setup("BlindGrasping", n)
    hb = pr.hip(sc, ms)
    core = hb.core
    hb.reset()
    core.refresh_body_states()
    torch.cuda.synchronize()
    rbs = core.rigid_body_states.cpu().numpy()
    sp = hb.get("site_pose")
    hbi = model.hand_local_rigid_body_index
    np.testing.assert_allclose(rbs[:, hbi, :7], sp[0:7].T, atol=1e-6)
    for f in range(5):
        np.testing.assert_allclose(rbs[:, model.fingertip_local_indices[f], :7], sp[7 * (1 + f):7 * (2 + f)].T, atol=1e-6)
        np.testing.assert_allclose(rbs[:, model.fingerpad_local_indices[f], :7], sp[7 * (6 + f):7 * (7 + f)].T, atol=1e-6)
    np.testing.assert_allclose(rbs[:, -1, :3], hb.get("box_pos").T, atol=1e-7)
    np.testing.assert_allclose(core.dof_state.cpu().numpy()[:, :, 0], hb.get("q").T, atol=0)
    # set_dof_state_tensor_indexed: only the listed envs change
    before = hb.get("q").copy()
    core.dof_state[:, :, 0] = 0.123
    core.set_dof_state_indexed(torch.tensor([1, 65]))
    after = hb.get("q")
    assert np.allclose(after[:, [1, 65]], 0.123) and np.allclose(np.delete(after, [1, 65], 1), np.delete(before, [1, 65], 1))


def test_make_env_product_path_on_gpu():
    """The product's own surface (make_env -> DexHandEnv -> C-ABI) on the GPU, against the oracle driven with the
    same actions and the same Philox reset stream; plus the extras / obs_dict contract."""
    import torch
    from dexrobot_isaac_amd import default_cfg, make_env
    from oracle.py_backend import OracleCore
    n = 96
    cfg = default_cfg("BlindGrasping")
    cfg["env"]["episodeLength"] = 12
    env = make_env("BlindGrasping", n, "cuda:0", "cuda:0", 0, cfg=cfg)
    ref = make_env("BlindGrasping", n, "cpu", "cpu", 0, cfg=cfg, _core_factory=OracleCore)
    o_g, o_r = env.reset(), ref.reset()
    assert o_g.is_cuda and o_g.shape == (n, 158)
    np.testing.assert_allclose(o_g.cpu().numpy(), o_r.numpy(), atol=2e-4)
    g = torch.Generator().manual_seed(5)
    for t in range(16):
        a = 2 * torch.rand(n, 18, generator=g) - 1
        og, rg, dg, ig = env.step(a.cuda())
        orr, rr, dr, ir = ref.step(a)
        np.testing.assert_allclose(og.cpu().numpy(), orr.numpy(), atol=2e-3)
        np.testing.assert_allclose(rg.cpu().numpy(), rr.numpy(), atol=2e-2, rtol=1e-4)
        assert (dg.cpu() == dr).all() and dg.dtype == torch.bool
        assert float(ig["timeout_rate"]) == float(ir["timeout_rate"])
        for k in ("success", "failure", "timeout", "failure_reason_hitting_ground"):
            assert (ig[k].cpu() == ir[k]).all()
        assert (ig["episode_length"].cpu() == ir["episode_length"]).all()
    assert int(env.reset_buf.sum()) + int(env.episode_step_count.sum()) > 0
    assert float(ig["reward_components"]["termination_timeout_penalty_weighted"].min()) <= 0
    od = env.get_observations_dict()
    cat = torch.cat([od[k] for k in env.task_cfg["policy_observation_keys"]], dim=1)
    assert torch.allclose(cat, env.obs_buf)
    rbs = env.rigid_body_states
    assert rbs.shape == (n, 38, 13) and torch.allclose(rbs[:, 6, :7], od["hand_pose"], atol=1e-6)
    assert env.contact_forces.shape == (n, 5, 3)
    env.reset_idx(torch.tensor([3, 5], device="cuda:0"))
    assert env.episode_step_count[[3, 5]].tolist() == [0, 0]
    env.close()


def test_long_random_rollout_stays_finite_and_resets_cycle():
    """BASELINE configs[2] shape at reduced N: 700 random-action control steps; state must stay finite, joints inside
    their limits, the box on or above the ground, and the episode machinery must cycle (stage-1 failures at t = 4 s)."""
    import torch
    from dexrobot_isaac_amd import make_env
    n = 1024
    env = make_env("BlindGrasping", n, "cuda:0", "cuda:0", 0)
    env.reset()
    g = torch.Generator(device="cuda:0").manual_seed(1)
    resets = 0
    for t in range(700):
        obs, rew, done, info = env.step(2 * torch.rand(n, 18, device="cuda:0", generator=g) - 1)
        resets += int(done.sum())
    assert torch.isfinite(obs).all() and torch.isfinite(rew).all()
    q = env.dof_pos
    lo, hi = env.dof_props[:, 4], env.dof_props[:, 5]
    assert (q >= lo - 1e-5).all() and (q <= hi + 1e-5).all()
    box_z = env.actor_root_state_tensor[:, 1, 2]
    assert (box_z > 0.015).all() and (box_z < 0.6).all()
    assert resets >= 2 * n                       # every env failed the pre-grasp check at least twice
    assert float(info["failure_rate"]) >= 0.0 and int(env.episode_step_count.max()) <= 499
    env.close()


def test_domain_randomisation_stress_config5():
    """BASELINE configs[4]: per-env box mass / friction randomisation (new capability; ranges are this build's choice).
    The device Philox draw must equal the oracle's, masses must show up as ground reaction m*g, and the run stays finite."""
    import torch
    from dexrobot_isaac_amd import make_env
    from oracle.oracle import Oracle
    n = 512
    dr = {"mass": (0.05, 0.2), "friction": (0.5, 1.5), "seed": 4242}
    env = make_env("BlindGrasping", n, "cuda:0", "cuda:0", 0, domain_randomisation=dr)
    core = env._core
    mass, mu = core.field("box_mass")[0].cpu().numpy(), core.field("box_mu")[0].cpu().numpy()
    assert 0.05 <= mass.min() and mass.max() <= 0.2 and mass.std() > 0.03
    assert 0.5 <= mu.min() and mu.max() <= 1.5 and mu.std() > 0.2
    sc, model = build_sim_config(env.cfg, dr=dr)
    o = Oracle(sc, model.to_struct())
    np.testing.assert_allclose(o.get("box_mass")[0], mass, rtol=5e-7)     # same Philox draw (fma contraction: 1 ulp)
    env.reset()
    g = torch.Generator(device="cuda:0").manual_seed(3)
    for _ in range(60):
        obs, rew, done, _ = env.step(0.2 * (2 * torch.rand(n, 18, device="cuda:0", generator=g) - 1))
    assert torch.isfinite(obs).all()
    fz = core.field("cforce")[3 * 16 + 2].cpu().numpy()          # ground reaction on the resting boxes
    rest = np.abs(core.field("box_lin").cpu().numpy()).max(axis=0) < 1e-3
    assert rest.mean() > 0.9
    np.testing.assert_allclose(fz[rest], 9.81 * mass[rest], rtol=2e-2)
    env.close()


def test_action_sweep_like_reference_harness():
    """The reference's smoke procedure (examples/dexhand_test.py:1470-1584, 1707-1782) as an automated test:
    BaseTask, position control, every finger action swept -1 -> 1 -> -1 over 100 steps (base actions 0 -> -1 -> 1 -> 0,
    scaled 0.5); coupled joints must move together, r_f_joint3_1 must stay at 0 and the hand must come back to its
    initial pose within 0.1 rad."""
    import torch
    from dexrobot_isaac_amd import default_cfg, make_env
    cfg = default_cfg("BaseTask")
    cfg["task"]["controlMode"] = "position"
    cfg["env"]["episodeLength"] = 5000
    env = make_env("BaseTask", 2, "cuda:0", "cuda:0", 0, cfg=cfg)
    env.reset()
    a = torch.zeros(2, 18, device="cuda:0")
    a[:, 6:] = -1.0
    for _ in range(60):                                           # settle at the closed pose
        env.step(a)
    q0 = env.dof_pos.clone()
    moved = torch.zeros(26, device="cuda:0")
    for idx in range(12):
        for s in range(100):
            a[:, :6] = 0.0
            a[:, 6:] = -1.0
            b = idx % 6
            bv = -(s / 24.0) if s < 25 else (-1.0 + 2.0 * (s - 25) / 49.0 if s < 75 else 1.0 - (s - 75) / 24.0)
            fv = -1.0 + 2.0 * s / 49.0 if s < 50 else 1.0 - 2.0 * (s - 50) / 49.0
            a[:, b] = 0.5 * bv
            a[:, 6 + idx] = fv
            env.step(a)
            d = (env.dof_pos[0] - q0[0]).abs()
            moved = torch.maximum(moved, d)
            if idx == 2 and s == 49:                              # th_dip drives joints 1_3 and 1_4 together
                assert abs(float(env.dof_pos[0, 8] - env.dof_pos[0, 9])) < 0.05 and float(d[8]) > 0.3   # 50 steps x 0.01 rad/step cap
            if idx == 3 and s == 49:                              # ff_spr: 5_1 = 2 x (2_1, 4_1); 3_1 fixed
                q = env.dof_pos[0]
                assert abs(float(q[10] - q[18])) < 0.02 and abs(float(q[22] - 2 * q[10])) < 0.04 and float(q[10]) > 0.15
    assert float(moved[14]) < 0.02                                # r_f_joint3_1 is held at 0 (target 0, only dynamic coupling)
    assert (moved[[6, 7, 8, 9, 10, 11, 12, 13, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25]] > 0.15).all()   # every other finger DOF moved
    for _ in range(60):
        a[:, :6] = 0.0
        a[:, 6:] = -1.0
        env.step(a)
    assert float((env.dof_pos[0] - q0[0]).abs().max()) < 0.1      # "Hand returned close to initial position"
    assert torch.isfinite(env.obs_buf).all()
    env.close()


def test_custom_post_action_filter_and_coupling_rule_host_path():
    """register_post_action_filter / set_coupling_rule (action_processor.py:698-720): with a custom filter enabled or a
    custom coupling rule set, the action stage runs on the host (torch) and the staged device path does the rest.  An
    identity filter plus a coupling rule that restates the table must reproduce the fused single-launch step; a filter
    that halves the commanded change must show up in the targets."""
    import torch
    from dexrobot_isaac_amd import make_env
    from dexrobot_isaac_amd.config import default_cfg

    def mk():
        cfg = default_cfg("BlindGrasping")
        cfg["env"]["numEnvs"] = 128
        return make_env("BlindGrasping", 128, "cuda:0", "cuda:0", 0, cfg=cfg)

    ref, env = mk(), mk()
    ap = env.action_processor
    ap.register_post_action_filter("identity", lambda prev, rule, tgt: tgt)
    ap._enabled_post_action_filters = ap._enabled_post_action_filters + ["identity"]   # dexhand_base.py:255-261
    tbl_ctrl, tbl_dof, tbl_scale = ap._cpl_ctrl.clone(), ap._cpl_dof.clone(), ap._cpl_scale.clone()

    def coupling(active):
        full = torch.zeros(active.shape[0], 26, device=active.device)
        full[:, :6] = active[:, :6]
        full[:, tbl_dof] = active[:, tbl_ctrl] * tbl_scale
        return full
    ap.set_coupling_rule(coupling)
    assert ap._host_path() and not ref.action_processor._host_path()
    ref.reset(); env.reset()
    g = torch.Generator(device="cuda:0").manual_seed(7)
    for t in range(12):
        a = 2 * torch.rand(128, 18, device="cuda:0", generator=g) - 1
        o1, r1, d1, _ = ref.step(a)
        o2, r2, d2, _ = env.step(a)
        torch.testing.assert_close(env.full_dof_targets, ref.full_dof_targets, atol=1e-6, rtol=1e-6)
        torch.testing.assert_close(o2, o1, atol=2e-4, rtol=1e-4)
        assert bool((d1 == d2).all())
    # a filter that halves the step towards the raw target
    ap.register_post_action_filter("half", lambda prev, rule, tgt: prev + 0.5 * (tgt - prev))
    ap._enabled_post_action_filters = ["velocity_clamp", "position_clamp", "half"]
    ap.set_coupling_rule(None)
    prev = ap.active_prev_targets.clone()
    prev_ref = ref.action_processor.active_prev_targets.clone()
    a = torch.ones(128, 18, device="cuda:0")
    env.step(a); ref.step(a)
    d_env = (ap.active_prev_targets - prev)[:, :6]
    d_ref = (ref.action_processor.active_prev_targets - prev_ref)[:, :6]
    torch.testing.assert_close(d_env, 0.5 * d_ref, atol=1e-6, rtol=1e-5)


def test_step_timing_and_step_stage_entry_points():
    """dexsim_step_timing (in-situ hipEvent pairs around the step launch) and DEXSIM_STAGE_STEP (re-launch of the
    production kernel with the last action pointer) behave as declared in include/dexsim.h."""
    import torch
    from dexrobot_isaac_amd import _abi
    from dexrobot_isaac_amd.core import DexSimCore
    sc, _, ms = pr.setup("BlindGrasping", 256)
    core = DexSimCore(sc, ms, "cuda:0")
    core.reset()
    a = 2 * torch.rand(256, 18, device="cuda:0") - 1
    core.step_timing(True)
    for _ in range(5):
        core.step(a)
    us, n = core.step_timing(False)
    assert n == 5 and 10.0 < us < 5000.0
    q0 = core.field("q").clone()
    core.run_stage(_abi.STAGE["STEP"])               # advances the simulation by one control step (minus the gated launch)
    torch.cuda.synchronize()
    assert torch.isfinite(core.obs_buf).all() and not torch.equal(core.field("q"), q0)
    t = core.time_stage(_abi.STAGE["PHYSICS"], 3)
    assert t > 0


@pytest.mark.parametrize("near_box", [False, True, "box_alone", "hand_on_box"], ids=["hand_clear", "contacts", "tumbled_box_alone", "hand_on_tumbled_box"])
def test_fused_physics_launch_equals_four_single_substep_launches(near_box):
    """k_physics4 inlines the sub-step body four times; four k_physics1 launches run the same body once each.  State after
    one sim.dt must be bit-identical (the early box solve splits its sweeps around a barrier but performs the same
    arithmetic sequence; contact forces do not feed back).  The tumbled samples (tests/tumbled_states.py, N = 256) add corner
    lists other than 0-3, slots that change their corner within the four sub-steps, and edge / vertex hand contacts."""
    import torch
    from dexrobot_isaac_amd import _abi
    tumbled = isinstance(near_box, str)
    n = 256 if tumbled else 192
    sc, model, ms = pr.setup("BlindGrasping", n)
    a, b = pr.hip(sc, ms), pr.hip(sc, ms)
    st = pr.tumbled_state(near_box, n) if tumbled else pr.random_state(np.random.default_rng(23), model, n, near_box=near_box)
    pr.load(a, st), pr.load(b, st)
    a.core.run_stage(_abi.STAGE["PHYSICS"])
    for _ in range(4):
        b.core.run_stage(_abi.STAGE["SUBSTEP"])
    torch.cuda.synchronize()
    for f in ("q", "qd", "box_pos", "box_quat", "box_lin", "box_ang", "site_pose", "ncontact", "cforce"):
        assert np.array_equal(a.get(f), b.get(f)), f


def test_env_actions_copy_written_by_the_step_kernel():
    """env.actions (DexHandBase.actions = actions.clone()) is filled by the action block of the step kernel."""
    import torch
    from dexrobot_isaac_amd import make_env
    from dexrobot_isaac_amd.config import default_cfg
    cfg = default_cfg("BlindGrasping")
    cfg["env"]["numEnvs"] = 100
    env = make_env("BlindGrasping", 100, "cuda:0", "cuda:0", 0, cfg=cfg)
    env.reset()
    a = 2 * torch.rand(100, 18, device="cuda:0") - 1
    keep = a.clone()
    env.step(a)
    a.zero_()                                  # the caller may reuse its tensor right away
    torch.cuda.synchronize()
    assert torch.equal(env.actions, keep)


def test_step_sink_writes_rollout_rows():
    """dexsim_set_step_sink / RolloutBuffer.sink: the step's flush writes obs, reward and done also into the rollout slot."""
    import torch
    from dexrobot_isaac_amd.core import DexSimCore
    from dexrobot_isaac_amd.rollout import RolloutBuffer
    n = 200                                              # not a multiple of 64: exercises the partial last workgroup
    sc, _, ms = pr.setup("BlindGrasping", n, **{"env.episodeLength": 6})
    core = DexSimCore(sc, ms, "cuda:0")
    core.reset()
    rb = RolloutBuffer(8, n, int(sc.num_obs), "cuda:0")
    g = torch.Generator(device="cuda:0").manual_seed(11)
    for t in range(8):
        a = 2 * torch.rand(n, 18, device="cuda:0", generator=g) - 1
        rb.sink(core)
        core.step(a)
        torch.cuda.synchronize()
        assert torch.equal(rb.slots[0].obs[t], core.obs_buf)
        assert torch.equal(rb.slots[0].rew[t], core.rew_buf)
        assert torch.equal(rb.slots[0].done[t].bool(), core.reset_buf.bool())
        assert torch.equal(rb.slots[0].stats[t, :20], core.stats[:20])     # dexsim_set_stats_sink: the step's statistics block
    assert rb.full() and int(rb.slots[0].done.sum()) > 0   # timeouts at step 5 really reached the sink
    h = rb.gather_async()
    obs, rew, done = h()
    assert obs.shape == (8, n, int(sc.num_obs))
    st = h.stats()                                         # single rank: the whole population is this rank's shard
    assert float(st["timeout_rate"].max()) == 1.0 and float(st["num_resets"].max()) == n and st["consecutive_successes"].tolist() == [0.0] * 8
    core.set_step_sink(None, None, None)
    core.set_stats_sink(None)
    before = rb.slots[0].obs[7].clone()
    core.step(a)
    torch.cuda.synchronize()
    assert torch.equal(rb.slots[0].obs[7], before)


def test_reset_gate_when_only_the_last_workgroup_resets():
    """The device-side reset gate is a step stamp (dexsim_device.h, CNT_ANY_RESET): nothing clears it, so a reset raised
    by the LAST workgroup of a grid that is larger than one residency wave (257 workgroups + a padded one) must still
    open the gated launch for every workgroup -- extra physics step for all envs, phase 1 of the reset for the flagged
    ones -- and the gate must close again in the following steps.  Checked against the oracle."""
    import torch
    n = 64 * 257 + 5
    sc, _, ms = pr.setup("BlindGrasping", n, **{"env.episodeLength": 40})
    o, hb = pr.backends(sc, ms, threads=8)
    obs_o, obs_h = o.reset(), hb.reset()
    es = np.zeros((1, n))
    es[0, 64 * 257:] = 37                                    # the five envs of the last (padded) workgroup time out at step 1
    o.set("episode_step", es)
    hb.set("episode_step", es)
    rng = np.random.default_rng(11)
    for t in range(3):
        a = (2 * rng.random((n, 18)) - 1).astype(np.float32)
        oo, ro, do = o.step(a)
        oh, rh, dh = hb.step(a)
        st_h, st_o = hb.stats(), o.stats()
        assert st_h[16] == st_o[16] == (5 if t == 1 else 0)                  # resets in this step
        assert st_h[17] == (2 if t == 1 else 1)                              # physics steps in this step
        assert (do == dh.astype(bool)).all() and do.sum() == (5 if t == 1 else 0)
        np.testing.assert_allclose(oh, oo, atol=2e-3)
        if t == 1:
            # phase 1 ran for the flagged envs (observer state zeroed after the extra physics step) ...
            assert (hb.get("prev_actions")[:, 64 * 257:] == 0).all() and (hb.get("prev_dof_pos")[:, 64 * 257:] == 0).all()
            assert (hb.get("reset_count")[0, 64 * 257:] == 2).all() and (hb.get("reset_count")[0, :64 * 257] == 1).all()
            # ... and the extra physics step ran for ALL envs, first workgroup included
        np.testing.assert_allclose(hb.get("q")[:, :64], o.get("q")[:, :64], atol=5e-4)
        np.testing.assert_allclose(hb.get("q")[:, -5:], o.get("q")[:, -5:], atol=5e-4)
        assert abs(st_h[18] - st_o[18]) < 0.01 and abs(st_h[19] - st_o[19]) < 0.01   # mean contacts (total, hand) of the main step


def test_config2_base_task_position_1024_free_running():
    """BASELINE configs[1] at its stated shape: BaseTask, num_envs=1024, position control, no object (articulated
    forward dynamics only), 30 free-running control steps with random actions against the oracle.  No contacts, so the
    trajectories do not bifurcate: every env is compared, max error over all envs and steps."""
    n = 1024
    sc, _, ms = pr.setup("BaseTask", n, **{"task.controlMode": "position"})
    o, hb = pr.backends(sc, ms, threads=8)
    np.testing.assert_allclose(hb.reset(), o.reset(), atol=2e-5)
    rng = np.random.default_rng(21)
    worst_obs = worst_rew = 0.0
    for t in range(30):
        a = (2 * rng.random((n, 18)) - 1).astype(np.float32)
        oo, ro, do = o.step(a)
        oh, rh, dh = hb.step(a)
        assert (do == dh.astype(bool)).all()
        worst_obs = max(worst_obs, float(np.abs(oh - oo).max()))
        worst_rew = max(worst_rew, float(np.abs(rh - ro).max()))
    # velocities are finite differences of q over control_dt = 0.01 s (x100), q itself agrees to ~1e-5
    assert worst_obs < 5e-3 and worst_rew < 1e-3, (worst_obs, worst_rew)
    np.testing.assert_allclose(hb.get("q"), o.get("q"), atol=5e-5)
    assert o.get("ncontact").max() == 0 and hb.get("ncontact").max() == 0


def test_config5_dr_8192_with_reset_churn():
    """BASELINE configs[4] at its stated shape: num_envs=8192, per-env box mass / friction randomisation, episode clocks
    staggered so that some env resets in every control step (reset_idx churn: the device-gated second physics step runs
    every step), 30 control steps with random actions against the oracle on the same device/host Philox streams.  The bar
    is the free-running one: exact integer bookkeeping for envs that did not bifurcate, statistical for trajectories."""
    n = 8192
    cfg = default_cfg("BlindGrasping")
    cfg["env"]["numEnvs"] = n
    dr = {"mass": (0.05, 0.2), "friction": (0.5, 1.5), "seed": 4242}
    sc, model = build_sim_config(cfg, dr=dr)
    o, hb = pr.backends(sc, model.to_struct(), threads=16)
    np.testing.assert_allclose(hb.get("box_mass"), o.get("box_mass"), rtol=5e-7)
    np.testing.assert_allclose(hb.get("box_mu"), o.get("box_mu"), rtol=5e-7)
    np.testing.assert_allclose(hb.reset(), o.reset(), atol=2e-4)
    rng = np.random.default_rng(31)
    k = rng.integers(173, 200, (1, n))                      # stage-1 clocks: every env fails the pre-grasp check within 30 steps
    for b in (o, hb):
        b.set("episode_step", k)
        b.set("time_in_stage", k * float(sc.control_dt))
    errs, mism, resets = [], 0, 0
    for t in range(30):
        a = (2 * rng.random((n, 18)) - 1).astype(np.float32)
        oo, ro, do = o.step(a)
        oh, rh, dh = hb.step(a)
        errs.append(np.abs(oh - oo).max(axis=1))
        mism += int((do != dh.astype(bool)).sum())
        assert abs(hb.stats()[16] - o.stats()[16]) <= 2     # resets this step
        assert hb.stats()[17] == (2 if do.any() else 1)
        resets += int(do.sum())
    errs = np.stack(errs)
    assert np.median(errs) < 1e-4 and np.percentile(errs, 99) < 5e-3, (np.median(errs), np.percentile(errs, 99))
    assert mism <= 8 and resets >= n                         # every env was reset once; <0.01 % done-flag bifurcations
    assert (np.abs(hb.get("reset_count") - o.get("reset_count")).sum()) <= 8
    assert np.isfinite(hb.obs_buf()).all()


def test_hip_error_is_a_small_multiple_of_fp32_roundoff():
    """Derives the physics tolerance instead of asserting it: the same teacher-forced sub-step on the fp64 oracle, the
    fp32 oracle (dense Cholesky) and the HIP kernels (block/Schur factorisation, fp32).  For every field the HIP error
    against fp64 must stay within a small multiple c of the fp32 oracle's own error against fp64, at the 99.9th percentile
    and at the maximum, over the envs whose contact sets agree in all three (a contact appearing or not is a discontinuity,
    not roundoff)."""
    n = 512
    sc, model, ms = pr.setup("BlindGrasping", n)
    o64, o32, hb = pr.backends(sc, ms, f64=True)
    rng = np.random.default_rng(41)
    report = {}
    for trial, near in enumerate((True, False, True)):
        st = pr.random_state(rng, model, n, near_box=near)
        for b in (o64, o32, hb):
            pr.load(b, {k: np.asarray(v, dtype=np.float32) for k, v in st.items()})    # identical fp32-representable state everywhere
            b.substep(last=True)
        same = (o64.get("ncontact")[0] == o32.get("ncontact")[0]) & (o64.get("ncontact")[0] == hb.get("ncontact")[0])
        assert same.mean() > 0.97
        for f in ("q", "qd", "box_pos", "box_lin", "box_ang", "cforce"):
            pr.accumulate(report, f, o64.get(f), o32.get(f), hb.get(f), np.broadcast_to(same, o64.get(f).shape))
    # c = pr.C_RULE = 3 and the floors 1e-7 / 1e-6; measured: 1.0-1.5 with round 1's sequential solver, 1.2-2.7 with round 2's block
    # solver (the box twist goes through per-block copies and a sum over the blocks: profiles/round2_e/README.md)
    assert pr.C_RULE == 3.0
    pr.assert_c_rule(report, "random states, one teacher-forced sub-step each, n = 512")


@pytest.mark.parametrize("task,substeps", [("BlindGrasping", 4), ("BaseTask", 4), ("BlindGrasping", 2), ("BaseTask", 2),
                                            ("BlindGrasping", 6), ("BaseTask", 6)],
                         ids=["BlindGrasping", "BaseTask", "BlindGrasping-2", "BaseTask-2", "BlindGrasping-6", "BaseTask-6"])
def test_fused_step_equals_staged_step_bitwise(task, substeps):
    """dexsim_step (the physics launches with the action block on the first and the post block on 7 waves on the last, then
    the gated twin; with 4 sub-steps one launch each) against the three staged calls (k_actions, the physics launches without
    the blocks, k_post on 8 waves + the gated physics step) from identical state, over steps that include in-step resets:
    every output and the whole carried state must be BIT-identical.  k_actions runs the production action block itself, so
    this ties the fused production post block (7 waves, box-wave pre-tasks) to the stand-alone k_post that the golden
    replays exercise, and the action block inside a physics launch to the same block launched alone."""
    n = 200                                                  # 4 workgroups, the last one padded
    sc, _, ms = pr.setup(task, n, **{"env.episodeLength": 7, "sim.substeps": substeps})
    assert int(sc.substeps) == substeps
    _fused_equals_staged_bitwise(sc, ms, task, n)


def _fused_equals_staged_bitwise(sc, ms, task, n):
    import torch
    na = int(sc.num_actions)
    a, b = pr.hip(sc, ms), pr.hip(sc, ms)
    a.reset(); b.reset()
    g = torch.Generator(device="cuda:0").manual_seed(77)
    fields = ("q", "qd", "targets", "obs_all", "rew_comp", "rew", "reset_flag", "episode_step", "active_prev_targets",
              "prev_actions", "prev_dof_pos", "contact_duration_steps", "prev_contact_binary", "cforce", "cf5", "site_pose",
              "reset_count", "term_timeout", "failure_reason", "prev_finger_dof_vel", "prev_hand_vel") + \
             (("box_pos", "box_quat", "box_lin", "current_stage", "time_in_stage") if task == "BlindGrasping" else ())
    resets = 0
    for t in range(10):
        act = 2 * torch.rand(n, na, device="cuda:0", generator=g) - 1
        a.core.step(act)
        b.core.process_actions(act)
        b.core.physics_step(False)
        b.core.post_physics(False)
        torch.cuda.synchronize()
        assert torch.equal(a.core.obs_buf, b.core.obs_buf), t
        assert torch.equal(a.core.rew_buf, b.core.rew_buf) and torch.equal(a.core.reset_buf, b.core.reset_buf)
        assert torch.equal(a.core.dof_state, b.core.dof_state) and torch.equal(a.core.masks, b.core.masks)
        assert torch.equal(a.core.stats[:18], b.core.stats[:18])
        for f in fields:
            assert np.array_equal(a.get(f), b.get(f)), (t, f)
        resets += int(a.core.reset_buf.sum())
    assert resets >= n                                       # time-outs at step 6: the reset path was part of the comparison


def _golden_cfg(golden_dir, name, n, **over):
    """The resolved cfg of a golden scenario (its recorded cfg_overrides on the task defaults) for n envs."""
    from tests.l2_replay import scenario_config
    cfg = scenario_config(np.load(os.path.join(golden_dir, f"l2_{name}.npz"), allow_pickle=False), num_envs=n)
    cfg["env"].update(over)
    return cfg


@pytest.mark.parametrize("name,task,na,nobs", [("blind_cfg_fingers", "BlindGrasping", 12, 106), ("base_cfg_base", "BaseTask", 6, 82)])
def test_fused_step_equals_staged_step_bitwise_at_non_default_configurations(golden_dir, name, task, na, nobs):
    """test_fused_step_equals_staged_step_bitwise (same body, same fields) away from the defaults: the golden replays pin the
    stand-alone stages at these configurations, this ties the production step's fused action and post blocks to them.
    blind_cfg_fingers: fingers-only policy (12 actions), an 11-key permuted observation list with keys from neither default
    list, a failure-criteria subset, every threshold / decay / weight changed; base_cfg_base: base-only policy (6 actions),
    six non-default keys, changed velocity limits and weights.  N = 200, episodeLength 7, 10 steps with in-step resets."""
    n = 200
    sc, model = build_sim_config(_golden_cfg(golden_dir, name, n, episodeLength=7))
    assert (int(sc.num_actions), int(sc.num_obs), int(sc.episode_length)) == (na, nobs, 7)
    _fused_equals_staged_bitwise(sc, model.to_struct(), task, n)


@pytest.mark.parametrize("zero_targets", [False, True], ids=["targets", "zero_targets"])
@pytest.mark.parametrize("hand_base", [True, False], ids=["base_and_fingers", "fingers_only"])
@pytest.mark.parametrize("mode", ["position_delta", "position"])
def test_action_stage_matches_oracle(mode, hand_base, zero_targets):
    """dexsim_process_actions against the oracle's process_actions from a seeded random active_prev_targets /
    active_rule_targets state, N = 200 (the last workgroup padded).  fingers_only: task.policy_controls_hand_base = False,
    12 actions that drive the finger controls, the base controls follow their rule targets.  zero_targets: the
    pre-finalize_setup branch, every target 0 and active_prev_targets untouched.  actions, prev_actions, the action copy
    and every zero_targets output must match exactly; computed targets / active_prev_targets within 1e-6 abs (a target is at
    most two fp32 operations on values below 4 rad, so a contraction difference between hipcc and the C compiler stays
    below that)."""
    import torch
    n = 200
    sc, _, ms = pr.setup("BlindGrasping", n, **{"task.controlMode": mode, "task.policy_controls_hand_base": hand_base})
    na = int(sc.num_actions)
    assert na == (18 if hand_base else 12)
    rng = np.random.default_rng(13)
    lo, hi = np.array(sc.active_lower)[:, None], np.array(sc.active_upper)[:, None]
    prev = rng.uniform(lo, hi, (18, n)).astype(np.float32)
    state = {"active_prev_targets": prev, "active_rule_targets": np.clip(prev + rng.normal(0, 0.02, (18, n)), lo, hi),
             "targets": rng.uniform(-1, 1, (26, n)), "actions": rng.uniform(-1, 1, (18, n))}
    o, hb = pr.backends(sc, ms, {k: np.asarray(v, dtype=np.float32) for k, v in state.items()})
    copy = torch.full((n, na), 7.0, device="cuda:0")
    hb.core.set_action_copy(copy)
    act = rng.uniform(-1, 1, (n, na)).astype(np.float32)
    o.process_actions(act, zero_targets)
    hb.process_actions(act, zero_targets)
    torch.cuda.synchronize()
    a18 = np.zeros((18, n))
    a18[:na] = act.T
    for f in ("actions", "prev_actions"):
        assert np.array_equal(o.get(f), a18), f
        assert np.array_equal(hb.get(f), a18), f
    assert np.array_equal(copy.cpu().numpy(), act)
    tg = hb.get("targets")
    assert np.array_equal(hb.core.full_dof_targets.cpu().numpy().T.astype(np.float64), tg)
    if zero_targets:
        assert np.array_equal(o.get("targets"), np.zeros((26, n))) and np.array_equal(tg, np.zeros((26, n)))
        assert np.array_equal(o.get("active_prev_targets"), prev) and np.array_equal(hb.get("active_prev_targets"), prev)
    else:
        np.testing.assert_allclose(tg, o.get("targets"), rtol=0, atol=1e-6)
        np.testing.assert_allclose(hb.get("active_prev_targets"), o.get("active_prev_targets"), rtol=0, atol=1e-6)
        assert not np.array_equal(o.get("active_prev_targets"), prev)      # the step really moved the targets


def test_level2_gym_shim_matches_fused_step():
    """INTEGRATION.md level 2 (tests/dexsim_gym_shim.py: the gymapi subset of the reference's step path over the C-ABI):
    the reference-style sequence -- targets uploaded with set_dof_position_target_tensor, gym.simulate + fetch_results +
    refreshes, then the post-physics stage -- must reproduce the fused single-launch step bit for bit; the indexed
    setters must teleport exactly the listed envs."""
    import torch
    from tests.dexsim_gym_shim import DexSimGym
    n = 130
    sc, _, ms = pr.setup("BlindGrasping", n, **{"env.episodeLength": 6})
    a, gym = pr.hip(sc, ms), DexSimGym(sc, ms)
    b = gym.core
    a.reset(); b.reset()
    g = torch.Generator(device="cuda:0").manual_seed(5)
    for t in range(8):
        act = 2 * torch.rand(n, 18, device="cuda:0", generator=g) - 1
        a.core.step(act)
        # level 2: the action stage produces full_dof_targets (here the device stage; the reference's own Python would),
        # the upload goes through the gym call, then simulate / fetch / refresh, then the post-physics stage
        b.process_actions(act)
        gym.set_dof_position_target_tensor(None, b.full_dof_targets.clone())
        gym.simulate(None); gym.fetch_results(None, True)
        gym.refresh_dof_state_tensor(None); gym.refresh_actor_root_state_tensor(None)
        b.post_physics(False)
        torch.cuda.synchronize()
        assert torch.equal(a.core.obs_buf, b.obs_buf) and torch.equal(a.core.rew_buf, b.rew_buf), t
        assert torch.equal(a.core.reset_buf, b.reset_buf) and torch.equal(a.core.dof_state, gym.dof_state)
        assert torch.equal(a.core.root_state, gym.actor_root_state)
    assert int(a.core.field("reset_count").sum()) > n            # time-outs: the reset path was part of it
    gym.refresh_rigid_body_state_tensor(None)
    a.core.refresh_body_states()
    torch.cuda.synchronize()
    assert torch.equal(gym.rigid_body_state, a.core.rigid_body_states) and torch.equal(gym.net_contact_force, a.core.contact_forces_all)
    # indexed setters: global actor indices (2 actors per env: hand = 2 e, box = 2 e + 1)
    q_before = b.field("q").clone()
    gym.dof_state[:, :, 0] = 0.05
    gym.set_dof_state_tensor_indexed(None, gym.dof_state, torch.tensor([2 * 3, 2 * 129], dtype=torch.int32, device="cuda:0"), 2)
    torch.cuda.synchronize()
    q_after = b.field("q")
    assert torch.allclose(q_after[:, [3, 129]], torch.full((26, 2), 0.05, device="cuda:0"))
    keep = [i for i in range(n) if i not in (3, 129)]
    assert torch.equal(q_after[:, keep], q_before[:, keep])
    gym.actor_root_state[:, 1, :3] = torch.tensor([0.01, 0.02, 0.3], device="cuda:0")
    gym.set_actor_root_state_tensor_indexed(None, gym.actor_root_state, torch.tensor([2 * 7 + 1], dtype=torch.int32, device="cuda:0"), 1)
    torch.cuda.synchronize()
    assert torch.allclose(b.field("box_pos")[:, 7], torch.tensor([0.01, 0.02, 0.3], device="cuda:0"))


def test_saturated_contact_list_matches_oracle():
    """The whole contact list in use: hands lowered until fingers and palm lie on box and ground -- every env reaches
    DEXSIM_KMAX = 24 contacts (4 box/ground + 20 hand contacts in priority order, the rest truncated): every env's solver
    blocks are pairs of contacts and a workgroup has 768 work items, twice its item lanes (the generic variant of the sweeps,
    two rounds per pass).  Contact lists must be identical, the state after a full physics step within the teacher-forced
    tolerances."""
    from dexrobot_isaac_amd import _abi
    n = 192
    sc, _, ms = pr.setup("BlindGrasping", n)
    o, hb = pr.backends(sc, ms, pr.lowered_hand_state(np.random.default_rng(2), n, z=-0.42, dz=0.02, rot=0.15))
    o.substep(last=True)
    hb.substep(last=True)
    nc_o, nc_h = o.get("ncontact")[0], hb.get("ncontact")[0]
    assert (nc_o == nc_h).all() and nc_o.max() == _abi.KMAX and (nc_o > 16).mean() > 0.9
    for e in range(0, n, 7):
        pr.assert_same_entries(o.contacts(e), hb.contacts(e), atol=2e-6)
    np.testing.assert_allclose(hb.get("q"), o.get("q"), atol=2e-4)
    np.testing.assert_allclose(hb.get("qd"), o.get("qd"), atol=1e-2, rtol=5e-3)      # 24 coupled contacts: PGS amplifies roundoff
    np.testing.assert_allclose(hb.get("box_pos"), o.get("box_pos"), atol=2e-4)
    np.testing.assert_allclose(hb.get("cforce"), o.get("cforce"), atol=0.5, rtol=5e-2)
    # ... and three more full physics steps stay finite and in agreement on the list sizes
    for _ in range(3):
        o.physics_step()
        hb.physics_step()
    assert np.isfinite(hb.get("q")).all() and np.abs(hb.get("q") - o.get("q")).max() < 5e-3


@pytest.mark.parametrize("z", [-0.292, -0.30, -0.32], ids=["single-contact blocks, > 384 items", "some lanes with pairs", "mostly pairs"])
def test_generic_sweep_variants_match_oracle(z):
    """Between the common case (one contact per item lane, resident rows) and the saturated list: hands low enough for 8-14
    hand contacts per env, so that a workgroup has more work items than item lanes (384) and lanes with single-contact blocks
    sit next to lanes whose blocks are pairs.  One sub-step from identical state, then two free physics steps."""
    n = 128
    sc, _, ms = pr.setup("BlindGrasping", n)
    o, hb = pr.backends(sc, ms, pr.lowered_hand_state(np.random.default_rng(2), n, z=z, dz=0.004, rot=0.1))
    o.substep(last=True)
    hb.substep(last=True)
    nc_o, nc_h = o.get("ncontact")[0], hb.get("ncontact")[0]
    assert (nc_o == nc_h).all()
    nh = np.array([(o.contacts(e)[:, 8] != 2).sum() for e in range(n)])
    items = np.where(nh > 12, (nh + 1) // 2, nh).reshape(-1, 64).sum(1)          # solver blocks per workgroup
    assert items.max() > 384                                                      # more items than item lanes: rounds
    if z > -0.295:
        assert (nh <= 12).all()                                                   # no pairs anywhere: rounds of single contacts
    if z < -0.31:
        assert (nh > 12).mean() > 0.5
    np.testing.assert_allclose(hb.get("q"), o.get("q"), atol=2e-4)
    np.testing.assert_allclose(hb.get("qd"), o.get("qd"), atol=1e-2, rtol=5e-3)
    np.testing.assert_allclose(hb.get("box_pos"), o.get("box_pos"), atol=2e-4)
    np.testing.assert_allclose(hb.get("cforce"), o.get("cforce"), atol=0.5, rtol=5e-2)
    (_, tag_h, gen_h), (_, tag_o, gen_o) = hb.warm_cache(), o.warm_cache()
    assert (gen_h == gen_o).all() and (((tag_h >> 3) == gen_h) == ((tag_o >> 3) == gen_o)).all()   # the same cache slots written
    for _ in range(2):
        o.physics_step()
        hb.physics_step()
    assert np.isfinite(hb.get("q")).all() and np.abs(hb.get("q") - o.get("q")).max() < 5e-3


@pytest.mark.parametrize("substeps,iters", [(2, 8), (6, 16), (8, 32), (32, 32)],
                         ids=["physics=fast", "6 sub-steps (staged)", "8 sub-steps / 32 iterations", "physics=accurate"])
def test_other_substep_counts_match_oracle(substeps, iters):
    """cfg/physics/fast.yaml (substeps 2, 8 position iterations), a heavier setting in the direction of
    cfg/physics/accurate.yaml, and accurate.yaml itself at its real 32 sub-steps x 32 iterations (round 3; timed by
    `bench.py --substeps 32 --iterations 32`).  A physics step is substeps / 4 k_physics4 launches, then substeps % 4 k_physics1
    launches: the action block on the first launch, the post-physics block / reset tail on the last (32 sub-steps = 8 + 8
    launches, 2 sub-steps = 2 + 2, 6 = 3 + 3).  Whole control steps with in-step resets against the oracle; the integer
    bookkeeping must agree exactly."""
    n = 130
    sc, _, ms = pr.setup("BlindGrasping", n, **{"sim.substeps": substeps, "sim.physx.num_position_iterations": iters, "env.episodeLength": 8})
    assert int(sc.substeps) == substeps and int(sc.num_position_iterations) == iters
    o, hb = pr.backends(sc, ms)
    pr.control_steps(o, hb, np.random.default_rng(13), 12, reset_atol=2e-4, obs_bar=5e-3, rew_atol=2e-2, rew_rtol=1e-4, q_atol=5e-4)


def test_general_contact_path_is_bitwise_reproducible():
    """The block solver sums the blocks' velocity changes in a fixed order (reducers, no atomics) and deals work items by a
    prefix sum: two instances stepped through the same contact-rich state -- saturated lists first (generic sweep variant),
    then the common case -- must agree bit for bit, warm-start cache included."""
    import torch
    from dexrobot_isaac_amd.core import DexSimCore
    n = 1024
    sc, _, ms = pr.setup("BlindGrasping", n)
    outs = []
    for _ in range(2):
        core = DexSimCore(sc, ms, "cuda:0")
        core.reset()
        g = torch.Generator(device="cuda:0").manual_seed(3)
        q = core.field("q")
        q.zero_()
        q[2] = -0.40
        q[6:] = 0.3 * torch.rand(20, n, device="cuda:0", generator=g)
        core.field("qd").zero_()
        core.field("targets").copy_(q)
        for _ in range(40):
            core.physics_step(False)
        torch.cuda.synchronize()
        outs.append([core.field(f).clone() for f in ("q", "qd", "box_pos", "box_quat", "box_lin", "box_ang", "cforce", "wlam", "wgen", "ncontact")])
    assert outs[0][-1].float().mean() > 6 and outs[0][-1].max() > 8          # hands really rest on box and ground
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_debug_spin_build_never_hits_its_bound():
    """The LDS token waits of the sub-step kernel (box wave <- broadphase verdicts, Schur wave <- its helpers) are unbounded in
    the product build.  Its diagnostic twin (-DDEXSIM_DEBUG_SPIN, dexrobot_isaac_amd/build.py::build_debug_spin) bounds every
    wait and records a word in the counters block when one runs out: driven through the hand-clear and the general contact path
    it must record nothing and produce bit-identical results to the product build."""
    import json
    import subprocess
    import sys
    from dexrobot_isaac_amd.build import DEBUG_SPIN_LIB, LIB
    assert os.path.exists(DEBUG_SPIN_LIB), "build it with __graft_entry__.build() / build_debug_spin()"
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "debug_spin_child.py")
    res = {}
    for name, lib in (("product", LIB), ("debug", DEBUG_SPIN_LIB)):
        out = subprocess.run([sys.executable, child], env={**os.environ, "DEXSIM_LIB_PATH": lib}, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        res[name] = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["debug"]["spin_word"] == 0, f"a token wait ran into its bound: site/seq word {res['debug']['spin_word']:#x}"
    assert res["debug"]["hand_contacts"] > 4.0          # the general contact path really ran
    assert res["debug"]["digest"] == res["product"]["digest"]


@pytest.mark.gpu
def test_warm_start_generation_wrap_on_the_hip_path():
    """ADVICE round 2 (GPU half; CPU half: test_oracle_physics.py::test_warm_start_generation_wraps_...): two instances in the
    same contact-rich state, one with its warm-start generation moved right below the 2^27 wrap.  Across the wrap the
    kernels must go through bit-identical states (the cache keeps warming, box/ground and hand slots alike) and every tag
    stays a small positive integer."""
    import torch
    from dexrobot_isaac_amd import _abi
    from dexrobot_isaac_amd.core import DexSimCore
    n, wrap = 256, 1 << 27
    sc, _, ms = pr.setup("BlindGrasping", n)
    outs = []
    for gen0 in (1000, wrap - 30):
        core = DexSimCore(sc, ms, "cuda:0")
        core.reset()
        g = torch.Generator(device="cuda:0").manual_seed(3)
        q = core.field("q")
        q.zero_()
        q[2] = -0.40
        q[6:] = 0.3 * torch.rand(20, n, device="cuda:0", generator=g)
        core.field("qd").zero_()
        core.field("targets").copy_(q)
        for _ in range(60):
            core.physics_step(False)
        # move every env's generation to gen0; valid tags (8 * gen + corner) move with it, stale ones are dropped
        off, rows, _ = core.fields["wlam"]
        quad = core._arena_i32[off: off + rows * core.NS].view(_abi.NWKEY, core.NS, 4)
        gen = core.field("wgen")[0].clone()
        tag = quad[:, :n, 3]
        valid = (tag >> 3) == gen[None, :]
        quad[:, :n, 3] = torch.where(valid, 8 * gen0 + (tag & 7), torch.zeros_like(tag))
        core.field("wgen").fill_(gen0)
        nvalid0 = int(valid.sum().item())
        for _ in range(20):                       # 80 generations: the second instance crosses the wrap
            core.physics_step(False)
        torch.cuda.synchronize()
        tag = quad[:, :n, 3].clone()
        gen = core.field("wgen")[0]
        assert int(gen[0].item()) == (gen0 + 80) % wrap and bool((gen == gen[0]).all())
        assert int(tag.min().item()) >= 0 and int(tag.max().item()) < (1 << 30)
        nvalid = int(((tag >> 3) == gen[None, :]).sum().item())
        assert nvalid == int(core.field("ncontact").sum().item()) and nvalid0 > 4 * n     # one valid slot per contact, hand contacts among them
        outs.append([core.field(f).clone() for f in ("q", "qd", "box_pos", "box_quat", "box_lin", "box_ang", "cforce", "ncontact")]
                    + [quad[:, :n, :3].clone()])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_config3_headline_workload_as_itself_through_the_synchronous_reset():
    """BASELINE configs[2] as itself: BlindGrasping, num_envs = 4096, random actions, default
    config, 205 control steps from a fresh reset -- through the one event that defines the headline workload: at t = 4 s
    (control step 200) every env fails the stage-1 pre-grasp check and all 4096 reset IN THE SAME STEP (the device-gated
    second physics step runs exactly once).  HIP vs the oracle on the same actions and the same Philox reset stream.
    Tolerances: free-running bar (no hand contacts in this regime: the error does not grow through contacts) -- median obs
    error < 1e-4, 99.9th percentile < 5e-3 over ALL 205 steps; rewards 2e-2 abs; done flags, reset counts and physics-step
    counts exact."""
    n = 4096
    sc, _, ms = pr.setup("BlindGrasping", n)
    o, hb = pr.backends(sc, ms, threads=16)
    np.testing.assert_allclose(hb.reset(), o.reset(), atol=2e-4)
    rng = np.random.default_rng(2024)
    errs, sync_steps = [], []
    for t in range(205):
        a = (2 * rng.random((n, 18)) - 1).astype(np.float32)
        oo, ro, do = o.step(a)
        oh, rh, dh = hb.step(a)
        errs.append(np.abs(oh - oo).max(axis=1))
        assert (do == dh.astype(bool)).all(), t
        np.testing.assert_allclose(rh, ro, atol=2e-2, rtol=1e-4)
        assert hb.stats()[16] == o.stats()[16] and hb.stats()[17] == (2 if do.any() else 1)
        if do.any():
            sync_steps.append((t, int(do.sum())))
    # the synchronous all-env reset, exactly once: reset() evaluates the observations (and with them the stage clock) twice
    # (dexhand_base.py:805-838), so stage 1's 4 s run out in control step 199
    assert sync_steps == [(198, n)], sync_steps
    errs = np.stack(errs)
    assert np.median(errs) < 1e-4 and np.percentile(errs, 99.9) < 5e-3, (np.median(errs), np.percentile(errs, 99.9), errs.max())
    assert np.median(errs[199:]) < 1e-4                        # the new episodes start from the same Philox samples
    assert (hb.get("reset_count") == o.get("reset_count")).all() and int(o.get("reset_count").min()) == 2
    fr_h, fr_o = hb.get("failure_reason"), o.get("failure_reason")
    assert (fr_h == fr_o).all()
    assert float(hb.stats()[19]) == 0.0 and float(hb.stats()[18]) == 4.0     # the regime: no hand contact, the box on its 4 corners


@pytest.mark.gpu
def test_loaded_mjcf_with_perturbed_numbers_drives_the_hip_path():
    """f-3 on the GPU: a hand model with PERTURBED link lengths, masses, capsule radii, gains and joint
    ranges goes through export_mjcf -> load_mjcf -> make_env(hand_model=...) on the HIP path and is compared with the
    oracle driven by the same loaded model: the model's numbers are run-time data of the kernels, not constants compiled
    into them.  (No real DexHand MJCF exists offline -- absent submodule -- so the file is this build's own export.)
    Free-running control steps + a teacher-forced contact sub-step; the default model must give DIFFERENT outputs."""
    import torch
    from dexrobot_isaac_amd import default_cfg, make_env
    from dexrobot_isaac_amd.hand_model import HandModel
    from dexrobot_isaac_amd.mjcf import export_mjcf, load_mjcf
    from oracle.py_backend import OracleCore

    class Perturbed(HandModel):
        L_PROX = [0.043, 0.037, 0.049, 0.042, 0.030]
        L_MID = [0.027, 0.028, 0.025, 0.027, 0.023]
        L_DIST = [0.022, 0.024, 0.027, 0.020, 0.018]
        R_PROX = [0.0095, 0.0075, 0.0085, 0.0078, 0.0070]
        R_MID = [0.0080, 0.0080, 0.0070, 0.0072, 0.0066]
        R_DIST = [0.0075, 0.0066, 0.0074, 0.0068, 0.0061]
        M_PALM = 0.41
        M_LINK = [0.005, 0.012, 0.010, 0.006]
        PALM_CAP_R = 0.0135

    pm = Perturbed()
    pm.kp[6:] = 24.0
    pm.kd[6:] = 0.8
    pm.hi[7::4] = 0.9
    pm.armature[6:] = 2e-5
    loaded = load_mjcf(export_mjcf(pm))
    n = 128
    cfg = default_cfg("BlindGrasping")
    cfg["env"]["episodeLength"] = 14
    env = make_env("BlindGrasping", n, "cuda:0", "cuda:0", 0, cfg=cfg, hand_model=loaded)
    ref = make_env("BlindGrasping", n, "cpu", "cpu", 0, cfg=cfg, hand_model=loaded, _core_factory=OracleCore)
    dflt = make_env("BlindGrasping", n, "cuda:0", "cuda:0", 0, cfg=cfg)
    np.testing.assert_allclose(env.reset().cpu().numpy(), ref.reset().numpy(), atol=2e-4)
    dflt.reset()
    g = torch.Generator().manual_seed(11)
    worst = 0.0
    for t in range(18):
        a = 2 * torch.rand(n, 18, generator=g) - 1
        og, rg, dg, _ = env.step(a.cuda())
        orr, rr, dr, _ = ref.step(a)
        od, _, _, _ = dflt.step(a.cuda())
        worst = max(worst, float((og.cpu() - orr).abs().max()))
        assert (dg.cpu() == dr).all()
        np.testing.assert_allclose(rg.cpu().numpy(), rr.numpy(), atol=2e-2, rtol=1e-4)
    assert worst < 2e-3, worst
    assert float((og - od).abs().max()) > 1e-2               # the perturbed numbers really reached the kernels
    assert torch.allclose(env.dof_props.cpu(), torch.tensor(loaded.dof_props()))
    env.close(), dflt.close()
    # teacher-forced sub-step in a contact state (hands low over their boxes): contact lists and velocities vs the oracle
    sc, _ = build_sim_config({**cfg, "env": {**cfg["env"], "numEnvs": n}}, model=loaded)
    rng = np.random.default_rng(5)
    q = np.zeros((26, n))
    q[2] = rng.uniform(-0.43, -0.38, n)
    q[6:] = rng.uniform(0.0, 0.3, (20, n))
    o, hb = pr.backends(sc, loaded.to_struct(), dict(q=q, qd=0 * q, targets=q))
    for _ in range(3):
        o.substep(True); hb.substep(True)
    nc_o, nc_h = o.get("ncontact")[0], hb.get("ncontact")[0]
    same = nc_o == nc_h
    assert same.mean() > 0.97 and nc_o.mean() > 5.0
    np.testing.assert_allclose(hb.get("q")[:, same], o.get("q")[:, same], atol=2e-4)
    np.testing.assert_allclose(hb.get("qd")[:, same], o.get("qd")[:, same], atol=5e-3, rtol=2e-3)


@pytest.mark.gpu
def test_static_contact_test_box_of_the_reference_harness():
    """The reference's contact smoke procedure (examples/dexhand_test.py:950-1024: BaseTask + a STATIC 0.1 m box --
    gym.create_box, fix_base_link = True -- centred at (0.3, 0, 0.05) "beneath the middle finger"), f-4's last gap.  The
    box is `env.box = {fixed: true, size, position}`; the hand is driven over it and lowered through make_env().step() in
    `position` mode until the middle fingertip presses on the box top.  Asserts, on the HIP path and against the oracle: a
    contact force appears on the middle finger's distal link r_f_link3_4 (contact_forces[:, 2]) and nowhere else on the
    hand, contact_binary of the obs_dict follows it, the box does not move by a single bit, the root-state tensor has the
    second actor."""
    import torch
    from dexrobot_isaac_amd import default_cfg, make_env
    from oracle.py_backend import OracleCore
    cfg = default_cfg("BaseTask")
    cfg["task"]["controlMode"] = "position"
    cfg["env"]["episodeLength"] = 100000
    cfg["env"]["box"] = {"fixed": True, "size": 0.1, "position": [0.3, 0.0, 0.05], "friction": 1.0}
    n = 70
    env = make_env("BaseTask", n, "cuda:0", "cuda:0", 0, cfg=cfg)
    ref = make_env("BaseTask", n, "cpu", "cpu", 0, cfg=cfg, _core_factory=OracleCore)
    env.reset(), ref.reset()
    assert env.actor_root_state_tensor.shape == (n, 2, 13) and env.num_observations == 224
    box0 = env.actor_root_state_tensor[:, 1].clone()
    assert torch.allclose(box0[0, :7], torch.tensor([0.3, 0.0, 0.05, 0, 0, 0, 1.0], device="cuda:0"))
    lo, hi = env.action_processor.active_lower_limits, env.action_processor.active_upper_limits
    a = torch.zeros(n, 18)
    a[:, 6:] = -1.0                                             # fingers open (position mode: -1 = lower limit)
    x_t = torch.linspace(0.28, 0.32, n)                         # a little spread over the box top, all under the middle finger
    a[:, 0] = 2 * (x_t - float(lo[0])) / float(hi[0] - lo[0]) - 1
    z_t = -0.1925
    a[:, 2] = 2 * (z_t - float(lo[2])) / float(hi[2] - lo[2]) - 1
    for t in range(260):                                        # max_base_linear_velocity caps the approach
        og, _, _, _ = env.step(a.cuda())
        orr, _, _, _ = ref.step(a)
    cf_g, cf_r = env.contact_forces.cpu(), ref.contact_forces
    mag = cf_g.norm(dim=2)
    assert (mag[:, 2] > 5.0).all() and float(mag[:, [0, 1, 3, 4]].max()) == 0.0     # the middle finger, only
    np.testing.assert_allclose(cf_g.numpy(), cf_r.numpy(), rtol=2e-2, atol=0.2)
    od = env.get_observations_dict()
    assert (od["contact_binary"][:, 2] == 1).all() and float(od["contact_binary"][:, [0, 1, 3, 4]].sum()) == 0
    assert torch.equal(env.actor_root_state_tensor[:, 1], box0)                     # static: not a bit of motion
    np.testing.assert_allclose(og.cpu().numpy(), orr.numpy(), atol=2e-3)
    tip_z = od["fingertip_poses_world"][:, 7 * 2 + 2]
    assert float((tip_z - (0.1 + 0.007)).abs().max()) < 4e-3   # tip sphere (r = 7 mm) rests on the box top z = 0.1
    env.close()


@pytest.mark.gpu
def test_obs_dict_policy_mode_serves_policy_keys_from_obs_buf():
    """env.obsDict = 'policy' (dexsim_set_obs_dict_mode): the step no longer writes the 392 SoA rows behind
    get_observations_dict(); obs_dict serves the policy keys as views of obs_buf and refuses every other key of the reference's
    obs_dict with a message that says how to get it.  Everything the step returns is bit-identical to the default mode."""
    import torch
    from dexrobot_isaac_amd import default_cfg, make_env
    n = 130
    envs = []
    for mode in ("all", "policy"):
        cfg = default_cfg("BlindGrasping")
        cfg["env"]["episodeLength"] = 9
        cfg["env"]["obsDict"] = mode
        envs.append(make_env("BlindGrasping", n, "cuda:0", "cuda:0", 0, cfg=cfg))
    full, pol = envs
    full.reset(), pol.reset()
    g = torch.Generator().manual_seed(3)
    for t in range(14):
        a = (2 * torch.rand(n, 18, generator=g) - 1).cuda()
        of, rf, df, _ = full.step(a)
        op, rp, dp, ip = pol.step(a)
        assert torch.equal(of, op) and torch.equal(rf, rp) and torch.equal(df, dp)
    od_f, od_p = full.get_observations_dict(), pol.get_observations_dict()
    assert set(od_p) == set(pol.task_cfg["policy_observation_keys"])
    for k in od_p:
        assert torch.equal(od_p[k], od_f[k]), k
    assert torch.equal(torch.cat([od_p[k] for k in pol.task_cfg["policy_observation_keys"]], dim=1), pol.obs_buf)
    with pytest.raises(KeyError, match="obsDict"):
        od_p["all_finger_dof_pos"]
    assert float(pol._core.field("obs_all").abs().max()) == 0.0 and float(full._core.field("obs_all").abs().max()) > 0.0
    assert float(ip["reward_components"]["total"].abs().max()) > 0        # extras are unaffected
    with pytest.raises(RuntimeError, match="obsDict"):
        pol.action_processor.set_pre_action_rule(lambda prev, state: prev)
        pol.step(a)
    full.close(), pol.close()


@pytest.mark.gpu
def test_joint_limit_rows_match_oracle():
    """sim.dexsim_joint_limit_rows on the HIP path (general contact path: rows staged behind a finger's contacts, type-3 list
    entries, one-row blocks, warm-start slots 88 + ...) against the oracle: teacher-forced sub-steps from states in which many
    finger joints sit within the margin of a limit while the hand touches box and ground.  Lists identical entry by entry
    (type, capsule / joint level, gap), state to the usual teacher-forced tolerances, the limit rows' impulses to 2e-3 abs /
    2 % rel, statistics (rows are not contacts) exact; plus free-running control steps through dexsim_step."""
    n = 256
    sc, model, ms = pr.setup("BlindGrasping", n, **{"sim.dexsim_joint_limit_rows": True})
    assert int(sc.joint_limit_rows) == 1
    rng = np.random.default_rng(17)
    st = pr.random_state(rng, model, n)
    near = rng.random((20, n)) < 0.4                      # 40 % of the finger joints on / next to a limit
    side = rng.random((20, n)) < 0.7
    lo, hi = model.lo[6:, None], model.hi[6:, None]
    off = rng.uniform(0.0, 0.012, (20, n))
    st["q"][6:] = np.where(near, np.where(side, lo + off, hi - off), st["q"][6:])
    st["targets"][6:] = np.where(near, st["q"][6:] - np.where(side, 0.2, -0.2), st["targets"][6:])    # PD pushes into the stop
    o, hb = pr.backends(sc, ms, st)
    rows_seen = 0
    for sub in range(3):
        o.substep(last=True)
        hb.substep(last=True)
        nc_o, nc_h = o.get("ncontact")[0], hb.get("ncontact")[0]
        assert (nc_o == nc_h).all(), f"list length differs in {(nc_o != nc_h).sum()} envs at sub-step {sub}"
        for e in range(0, n, 4):
            co = o.contacts(e)
            pr.assert_same_entries(co, hb.contacts(e), atol=2e-6)
            rows_seen += int((co[:, 8] == 3).sum())
        np.testing.assert_allclose(hb.get("q"), o.get("q"), atol=2e-4)
        np.testing.assert_allclose(hb.get("qd"), o.get("qd"), atol=5e-3, rtol=2e-3)
        np.testing.assert_allclose(hb.get("cforce"), o.get("cforce"), atol=5e-2, rtol=2e-2)
        (lam_h, tag_h, gen_h), (lam_o, tag_o, gen_o) = hb.warm_cache(), o.warm_cache()
        vo, vh = (tag_o[88:] >> 3) == gen_o, (tag_h[88:] >> 3) == gen_h
        assert (vo == vh).all() and (gen_o == gen_h).all()
        lo3, lh3 = lam_o[88 * 3:].reshape(40, 3, n)[:, 0], lam_h[88 * 3:].reshape(40, 3, n)[:, 0]
        np.testing.assert_allclose(lh3[vo], lo3[vo], atol=2e-3, rtol=2e-2)
        pr.load(hb, {k: o.get(k) for k in pr.SYNC})
    assert rows_seen > n // 4 and float(np.abs(lo3[vo]).max()) > 1e-3       # rows exist and some carry load
    # free-running control steps through the production launch (dexsim_step), in-step resets included
    sc2, _, ms2 = pr.setup("BlindGrasping", 192, **{"sim.dexsim_joint_limit_rows": True, "env.episodeLength": 12})
    o2, h2 = pr.backends(sc2, ms2)
    np.testing.assert_allclose(h2.reset(), o2.reset(), atol=2e-4)
    for b in (o2, h2):                                      # hands low over their boxes: contacts from the first step on
        q = b.get("q")
        q[:6] = 0.0
        q[2] = -0.255
        q[6:] = 0.004                                       # fingers straight, next to their lower stops
        apt = b.get("active_prev_targets")
        apt[:] = 0.004
        apt[:6] = q[:6]
        b.set("q", q); b.set("targets", q); b.set("active_prev_targets", apt)
        b.set("box_pos", np.array([[0.0], [0.0], [0.0255]]) + 0 * q[:3])
    rng = np.random.default_rng(4)
    errs, mism, hand_max = [], 0, 0.0
    for t in range(16):
        a = (0.3 * (2 * rng.random((192, 18)) - 1)).astype(np.float32)
        oo, ro, do = o2.step(a)
        oh, rh, dh = h2.step(a)
        errs.append(np.abs(oh - oo).max(axis=1))
        mism += int((do != dh.astype(bool)).sum())
        assert h2.stats()[19] <= h2.stats()[18] and abs(h2.stats()[19] - o2.stats()[19]) < 0.05
        hand_max = max(hand_max, float(o2.stats()[19]))
    errs = np.stack(errs)
    assert np.median(errs) < 1e-4 and np.percentile(errs, 99) < 5e-3 and mism <= 2, (np.median(errs), np.percentile(errs, 99), mism)
    assert hand_max > 0.5                                   # (before the timeouts at step 11 send the hands back up)


@pytest.mark.gpu
def test_make_env_product_path_tight_without_contacts():
    """the only oracle comparison that went through make_env().step() carried bifurcation headroom
    (obs 2e-3, reward 2e-2) because fingers touch things in BlindGrasping.  The same product surface without contacts --
    BaseTask, position_delta, random actions, in-step resets by time-out -- at parity tolerances: obs 1e-4 abs, reward 1e-4
    abs + 1e-5 rel, done flags / extras masks / rates exact, 40 control steps."""
    import torch
    from dexrobot_isaac_amd import default_cfg, make_env
    from oracle.py_backend import OracleCore
    n = 200
    cfg = default_cfg("BaseTask")
    cfg["env"]["episodeLength"] = 17
    env = make_env("BaseTask", n, "cuda:0", "cuda:0", 0, cfg=cfg)
    ref = make_env("BaseTask", n, "cpu", "cpu", 0, cfg=cfg, _core_factory=OracleCore)
    np.testing.assert_allclose(env.reset().cpu().numpy(), ref.reset().numpy(), atol=1e-5)
    g = torch.Generator().manual_seed(8)
    resets = 0
    for t in range(40):
        a = 2 * torch.rand(n, 18, generator=g) - 1
        og, rg, dg, ig = env.step(a.cuda())
        orr, rr, dr, ir = ref.step(a)
        np.testing.assert_allclose(og.cpu().numpy(), orr.numpy(), atol=1e-4)
        np.testing.assert_allclose(rg.cpu().numpy(), rr.numpy(), atol=1e-4, rtol=1e-5)
        assert (dg.cpu() == dr).all()
        for k in ("success", "failure", "timeout"):
            assert (ig[k].cpu() == ir[k]).all()
        assert float(ig["timeout_rate"]) == float(ir["timeout_rate"]) and float(ig["failure_rate"]) == float(ir["failure_rate"])
        for k, v in ir["reward_components"].items():
            np.testing.assert_allclose(ig["reward_components"][k].cpu().numpy(), v.numpy(), atol=1e-4, rtol=1e-5, err_msg=k)
        resets += int(dr.sum())
    assert resets >= 2 * n
    env.close()


@pytest.mark.gpu
def test_make_env_product_path_at_a_non_default_configuration(golden_dir):
    """The product surface (make_env().step()) at the base_cfg_fingers configuration -- BaseTask, fingers-only policy (12
    actions), position mode, an 8-key non-default observation list, height and contact thresholds, finger velocity limit --
    against the oracle behind the same surface: obs 1e-4 abs, reward and every reward component 1e-4 abs + 1e-5 rel (the
    bounds of test_make_env_product_path_tight_without_contacts: no contacts here either), done flags / extras masks /
    episode_length exact, 12 steps with in-step resets at episodeLength 8.  A third env in env.obsDict = 'policy' mode returns
    the same bits as the default mode and serves the configured keys, concatenated, as obs_buf.  The action copy and the
    prev_actions segment of obs_buf (12 wide) hold the step's actions exactly."""
    import torch
    from dexrobot_isaac_amd import make_env
    from oracle.py_backend import OracleCore
    n = 96
    cfg = _golden_cfg(golden_dir, "base_cfg_fingers", n, episodeLength=8)
    keys = cfg["task"]["policy_observation_keys"]
    pcfg = _golden_cfg(golden_dir, "base_cfg_fingers", n, episodeLength=8, obsDict="policy")
    env = make_env("BaseTask", n, "cuda:0", "cuda:0", 0, cfg=cfg)
    pol = make_env("BaseTask", n, "cuda:0", "cuda:0", 0, cfg=pcfg)
    ref = make_env("BaseTask", n, "cpu", "cpu", 0, cfg=cfg, _core_factory=OracleCore)
    assert (env.num_actions, ref.num_actions, env.num_observations, ref.num_observations) == (12, 12, 85, 85)
    assert keys[2] == "prev_actions" and keys != default_cfg("BaseTask")["task"]["policy_observation_keys"]
    o0 = env.reset()
    np.testing.assert_allclose(o0.cpu().numpy(), ref.reset().numpy(), atol=1e-5)
    assert torch.equal(pol.reset(), o0)
    lo, hi = env.observation_encoder.component_slice_indices["prev_actions"]
    assert hi - lo == 12
    g = torch.Generator().manual_seed(21)
    resets = 0
    for t in range(12):
        a = 2 * torch.rand(n, 12, generator=g) - 1
        og, rg, dg, ig = env.step(a.cuda())
        op, rp, dp, _ = pol.step(a.cuda())
        orr, rr, dr, ir = ref.step(a)
        assert torch.equal(og, op) and torch.equal(rg, rp) and torch.equal(dg, dp)
        assert torch.equal(env.actions.cpu(), a) and torch.equal(og[:, lo:hi].cpu(), a) and torch.equal(orr[:, lo:hi], a)
        np.testing.assert_allclose(og.cpu().numpy(), orr.numpy(), atol=1e-4)
        np.testing.assert_allclose(rg.cpu().numpy(), rr.numpy(), atol=1e-4, rtol=1e-5)
        assert (dg.cpu() == dr).all()
        for k in ("success", "failure", "timeout"):
            assert (ig[k].cpu() == ir[k]).all()
        assert (ig["episode_length"].cpu() == ir["episode_length"]).all()
        assert set(ig["reward_components"]) == set(ir["reward_components"])
        for k, v in ir["reward_components"].items():
            np.testing.assert_allclose(ig["reward_components"][k].cpu().numpy(), v.numpy(), atol=1e-4, rtol=1e-5, err_msg=k)
        for e in (env, pol):
            od = e.get_observations_dict()
            assert torch.equal(torch.cat([od[k] for k in keys], dim=1), e.obs_buf)
        resets += int(dr.sum())
    assert set(pol.get_observations_dict()) == set(keys) and resets >= n
    env.close(), pol.close()
