"""Model structure folded out of the sub-step chains (template parameter MS of the step kernels, csrc/dexsim_physics.hip.inc::base_chain).

dexsim_create classifies the hand model's exact zeros and ones (base joints 4 and 5 sitting on joint 3 with axes e_y / e_z, unit
prismatic axes, flexion axes +-e_y) and launches step kernels whose chains leave those terms out.  DEXSIM_GENERAL_MODEL_PATH=1, read
once by dexsim_create, clears the classification: the same library then runs the general kernels.
  (1) the specialised kernels give the general kernels' values, compared with `==` over control steps and contact-rich physics steps;
  (2) a model that lacks one of the properties (by a small amount) runs the general code and still matches the oracle;
  (3) so does a model in which only some fingers lack them (the kernels are chosen for the whole model)."""
import numpy as np
import pytest

from tests.physics_rig import MODELS, backends, free_running, general_path, hip, setup

pytestmark = pytest.mark.gpu


def _snapshot(core):
    import torch
    torch.cuda.synchronize()
    out = {k: getattr(core, k).clone() for k in ("obs_buf", "rew_buf", "reset_buf")}
    for f in ("q", "qd", "box_pos", "box_quat", "box_lin", "box_ang", "ncontact", "clam"):
        if f in core.fields:
            out[f] = core.field(f).clone()
    off, rows, _ = core.fields["wlam"]                   # quad layout [key][env][4]: the padded lanes are sliced off
    out["wlam"] = core.arena[off: off + rows * core.NS].view(rows // 4, core.NS, 4)[:, : core.N].clone()
    return out


def _assert_same(a, b, where):
    for k in a:
        assert bool((a[k] == b[k]).all()), f"{where}: {k} differs in {int((a[k] != b[k]).sum())} words"


@pytest.mark.parametrize("task,n,over", [
    ("BlindGrasping", 133, {}),
    ("BlindGrasping", 133, {"sim.substeps": 2}),
    ("BaseTask", 64, {"task.controlMode": "position"}),
], ids=["default-133", "substeps2-133", "basetask-position-64"])
def test_specialised_forms_equal_the_general_forms(task, n, over):
    """Three workgroups, the last one padded (N = 133): 40 control steps from reset with random actions (hand-clear path and
    whatever the random hands touch), then 30 physics steps from the hands-on-boxes state of scripts/contact_regime.py (general
    contact path).  Every removed term is an exact zero and every removed factor an exact one: `==`, not a tolerance."""
    import torch
    from dexrobot_isaac_amd.core import DexSimCore
    sc, _, ms = setup(task, n, **over)
    spec = DexSimCore(sc, ms, "cuda:0")
    with general_path():
        gen = DexSimCore(sc, ms, "cuda:0")
    cores = (spec, gen)
    for c in cores:
        c.reset()
    _assert_same(_snapshot(spec), _snapshot(gen), "reset")
    g = torch.Generator(device="cuda:0").manual_seed(7)
    moved = 0.0
    for t in range(40):
        a = 2 * torch.rand(n, sc.num_actions, device="cuda:0", generator=g) - 1
        for c in cores:
            c.step(a)
        if t % 8 == 7 or t == 39:
            s = _snapshot(spec)
            _assert_same(s, _snapshot(gen), f"control step {t}")
            moved = max(moved, float(s["qd"].abs().max()))
    assert moved > 0.1                                   # the hands really moved
    g = torch.Generator(device="cuda:0").manual_seed(3)
    r = 0.3 * torch.rand(20, n, device="cuda:0", generator=g)
    for c in cores:
        q = c.field("q")
        q.zero_()
        q[2] = -0.40
        q[6:] = r
        c.field("qd").zero_()
        c.field("targets").copy_(q)
    for t in range(30):
        for c in cores:
            c.physics_step(False)
        if t % 10 == 9:
            s = _snapshot(spec)
            _assert_same(s, _snapshot(gen), f"physics step {t}")
    if sc.has_box:
        assert float(s["ncontact"].float().mean()) > 4.0  # hands really rest on box and ground
    for c in cores:
        c.close()


@pytest.mark.parametrize("name", list(MODELS))
def test_models_without_the_structure_match_the_oracle(name):
    """One model per property of the hand model's structure (tests/physics_rig.py::MODELS), each lacking it by a small amount (some of
    them properties the kernels do not rely on: those models run the specialised kernels), one lacking all, one with fingers of
    different shapes: 20 free-running control steps at N = 70 (two workgroups, one padded) against the CPU oracle at the bars of
    test_gpu_parity.py::test_free_running_steps_match_oracle (median obs error < 1e-4, 99th percentile < 5e-3, <= 2 done
    mismatches), and the same values with and without the switch."""
    sc, _, ms = setup("BlindGrasping", 70, model=name, **{"env.episodeLength": 12})      # (timeouts at 11)
    o, hb = backends(sc, ms)
    with general_path():
        hg = hip(sc, ms)
    free_running(o, hb, np.random.default_rng(3), 20, reset_atol=2e-4, median=1e-4, p99=5e-3, mismatches=2, resets=2, twin=hg, label=name)
    assert (hb.get("q") == hg.get("q")).all() and (hb.get("qd") == hg.get("qd")).all()
    hb.core.close(), hg.core.close()


