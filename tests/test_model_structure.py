"""Model structure folded out of the sub-step chains (template parameter MS of the step kernels, csrc/dexsim_physics.hip.inc::base_chain).

dexsim_create classifies the hand model's exact zeros and ones (base joints 4 and 5 sitting on joint 3 with axes e_y / e_z, unit
prismatic axes, flexion axes +-e_y) and launches step kernels whose chains leave those terms out.  DEXSIM_GENERAL_MODEL_PATH=1, read
once by dexsim_create, clears the classification: the same library then runs the general kernels.
  (1) the specialised kernels give the general kernels' values, compared with `==` over control steps and contact-rich physics steps;
  (2) a model that lacks one of the properties (by a small amount) runs the general code and still matches the oracle;
  (3) so does a model in which only some fingers lack them (the kernels are chosen for the whole model)."""
import contextlib
import math
import os

import numpy as np
import pytest

from dexrobot_isaac_amd.config import build_sim_config, default_cfg
from dexrobot_isaac_amd.hand_model import HandModel, rot_z

pytestmark = pytest.mark.gpu

SWITCH = "DEXSIM_GENERAL_MODEL_PATH"


@contextlib.contextmanager
def general_path():
    """dexsim_create inside the block clears the model classification."""
    old = os.environ.get(SWITCH)
    os.environ[SWITCH] = "1"
    try:
        yield
    finally:
        if old is None:
            del os.environ[SWITCH]
        else:
            os.environ[SWITCH] = old


def _cfg(task, n, **over):
    cfg = default_cfg(task)
    cfg["env"]["numEnvs"] = n
    for k, v in over.items():
        d = cfg
        parts = k.split(".")
        for p in parts[:-1]:
            d = d[p]
        d[parts[-1]] = v
    return cfg


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
    sc, model = build_sim_config(_cfg(task, n, **over))
    ms = model.to_struct()
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


# ---- models that lack the structure
def _tilt_axis(m, j):          # a flexion axis tilted by 1e-2 rad, renormalised
    a = np.array([0.0, -math.cos(1e-2), math.sin(1e-2)])
    m.jaxis[j] = a / np.linalg.norm(a)


def _break_poff4(m):
    m.jpoff[4] = (0.0, 2e-3, 0.0)


def _break_axis(m):
    _tilt_axis(m, 6 + 4 * 1 + 1)


def _break_qoff(m):
    j = 6 + 4 * 2 + 2
    m.jRoff[j] = m.jRoff[j] @ rot_z(1e-2)


def _break_com(m):
    m.com[6 + 4 * 3 + 2, 1] = 1e-3


def _break_all(m):
    _break_poff4(m), _break_axis(m), _break_qoff(m), _break_com(m)


def _mixed(m):                 # fingers 1 and 3 lack the structure, 2 and 4 (and the thumb) keep it
    m.com[6 + 4 * 1 + 3, 1] = 1e-3
    _tilt_axis(m, 6 + 4 * 3 + 2)


_ROT = (math.sin(0.05) / math.sqrt(2.0), math.sin(0.05) / math.sqrt(2.0), 0.0, math.cos(0.05))   # 0.1 rad about (1, 1, 0)
MODELS = {
    "poff4": (_break_poff4, None), "axis": (_break_axis, None), "qoff": (_break_qoff, None), "com": (_break_com, None),
    "hand_rot": (None, _ROT), "all": (_break_all, _ROT), "mixed": (_mixed, None),
}


@pytest.mark.parametrize("name", list(MODELS))
def test_models_without_the_structure_match_the_oracle(name):
    """One model per property of the hand model's structure, each lacking it by a small amount (some of them properties the kernels
    do not rely on: those models run the specialised kernels), one lacking all, one with fingers of different shapes: 20
    free-running control steps at N = 70 (two workgroups, one padded) against the CPU oracle at the bars of
    test_gpu_parity.py::test_free_running_steps_match_oracle (median obs error < 1e-4, 99th percentile < 5e-3, <= 2 done
    mismatches), and the same values with and without the switch."""
    from oracle.oracle import Oracle
    from tests.hip_backend import HipBackend
    edit, rot = MODELS[name]
    n = 70
    cfg = _cfg("BlindGrasping", n, **{"env.episodeLength": 12})
    if rot is not None:
        cfg["env"]["initialHandRot"] = list(rot)
    model = HandModel(cfg["env"]["initialHandPos"], cfg["env"]["initialHandRot"])
    if edit is not None:
        edit(model)
    sc, model = build_sim_config(cfg, model=model)
    ms = model.to_struct()
    o, hb = Oracle(sc, ms), HipBackend(sc, ms)
    with general_path():
        hg = HipBackend(sc, ms)
    obs_o, obs_h, obs_g = o.reset(), hb.reset(), hg.reset()
    np.testing.assert_allclose(obs_h, obs_o, atol=2e-4)
    assert (obs_h == obs_g).all()
    rng = np.random.default_rng(3)
    errs, mism = [], 0
    for t in range(20):
        a = (2 * rng.random((n, 18)) - 1).astype(np.float32)
        oo, ro, do = o.step(a)
        oh, rh, dh = hb.step(a)
        og, rg, dg = hg.step(a)
        assert (oh == og).all() and (rh == rg).all() and (dh == dg).all(), f"step {t}: the switch changes values"
        errs.append(np.abs(oh - oo).max(axis=1))
        mism += int((do != dh.astype(bool)).sum())
        assert abs(hb.stats()[16] - o.stats()[16]) <= 2      # resets this step
    errs = np.stack(errs)
    print(f"{name}: median {np.median(errs):.3g}  p99 {np.percentile(errs, 99):.3g}  done mismatches {mism}")
    assert np.median(errs) < 1e-4
    assert np.percentile(errs, 99) < 5e-3
    assert mism <= 2
    assert o.get("reset_count").sum() > n                    # resets (timeouts at 11) really happened
    assert (hb.get("q") == hg.get("q")).all() and (hb.get("qd") == hg.get("qd")).all()
    hb.core.close(), hg.core.close()
