"""The CPU oracle's L2 restatement against golden vectors produced by the reference's own Python
(tests/golden/generate_golden.py).  This is what PINS the oracle (prompt ③)."""
import json
import os

import numpy as np
import pytest

from dexrobot_isaac_amd.config import OBS_KEYS, REWARD_TERMS, build_sim_config, obs_key_offsets
from oracle.oracle import Oracle
from tests.l2_replay import replay, scenario_config

from tests.l2_replay import ALL_SCENARIOS as SCENARIOS  # noqa: E402


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, f"l2_{name}.npz"), allow_pickle=False)


@pytest.mark.parametrize("name", SCENARIOS)
def test_oracle_replays_reference_l2(golden_dir, name):
    npz = _load(golden_dir, name)
    sc, model = build_sim_config(scenario_config(npz))
    o = Oracle(sc, model.to_struct())
    err = replay(o, npz)
    assert err["obs"] < 2e-5
    # (replay also checks, on this backend: the end-of-scenario snapshot of the obs_dict components outside obs_buf and of
    # every reward component, the per-step success / failure / timeout rates and consecutive successes, and -- in the
    # round-2 scenarios -- explicit reset_idx(ids) events and per-step snapshots of every obs_dict key / reward component)
    assert any(k.startswith("final:") for k in err) and any(k.startswith("final_rc:") for k in err)
    if name in ("blind_wide", "base_wide"):
        assert any(k.startswith("ev:") for k in err) and any(k.startswith("snap:") for k in err)
    if "_cfg_" in name:       # non-default configurations: snapshots, every criterion's raw condition, the binary observations
        assert any(k.startswith("snap:") for k in err) and any(k.startswith("snap_rc:") for k in err)
        assert err["crit_fail"] == 0 and err["crit_succ"] == 0 and err["binaries"] == 0
        assert ("ev:targets" in err) == (name in ("blind_cfg_base", "base_cfg_base"))


def test_scenarios_cover_the_branches(golden_dir):
    """The fast scenario must actually exercise transitions, success, every failure type and timeouts."""
    npz = _load(golden_dir, "blind_fast")
    ts = npz["task_state"]
    assert (ts[:, 0] == 2).any() and (ts[:, 0] == 3).any()
    assert ts[:, 4].any() and ts[:, 5].any()
    assert npz["done"].sum() > 50
    assert (npz["rew"] > 1500).any()        # termination_success bonus paid
    assert (npz["rew"] < -150).any()        # failure / timeout penalty paid
    assert (npz["stats"][:, 0] > 0).any() and (npz["stats"][:, 1] > 0).any()
    base = _load(golden_dir, "base_default")
    assert base["done"].sum() == 12          # timeouts at episodeLength - 1
    # round 2: default-length FSM (stage 1 = 200 control steps) reaching stage 2, stage 3 and grasp_lift_success
    lng = _load(golden_dir, "blind_long")
    ts = lng["task_state"]
    assert (ts[:, 0] == 2).sum() > 20 and (ts[:, 0] == 3).sum() > 50 and (lng["rew"] > 1500).any()
    assert json.loads(str(lng["cfg_overrides"])) == {}
    # ... and two workgroups incl. a padded one, with explicit reset_idx events
    wide = _load(golden_dir, "blind_wide")
    assert int(wide["N"]) == 70 and len(wide["ev_step"]) == 2 and wide["done"].sum() > 200


CFG_SCENARIOS = [n for n in SCENARIOS if "_cfg_" in n]


def _get(cfg, dotted):
    d = cfg
    for p in dotted.split("."):
        d = d[p]
    return d


@pytest.mark.parametrize("name", CFG_SCENARIOS)
def test_cfg_scenarios_cover_their_branches(golden_dir, name):
    """The non-default scenarios (margins profile): every active failure criterion terminated an env, every deactivated
    criterion's condition was met in an env that went on, success was reached where a success criterion exists, and every
    binary observation took both values.  crit_fail / crit_succ are the raw conditions the reference's TerminationManager
    received; `done` and `stats` what it made of them."""
    from dexrobot_isaac_amd import _abi
    npz = _load(golden_dir, name)
    cfg = scenario_config(npz)
    sc, _ = build_sim_config(cfg)
    blind = str(npz["task"]) == "BlindGrasping"
    crit, done = npz["crit_fail"].astype(bool), npz["done"].astype(bool)       # [T][5][N], [T][N]
    avail = range(_abi.NUM_FAIL) if blind else [0]
    for i in avail:
        if sc.active_failure_mask >> i & 1:
            assert (crit[:, i] & done).any(), f"{_abi.FAILURE_CRITERIA[i]} never terminated an env"
            assert (~crit[:, i]).any()
        else:
            assert (crit[:, i] & ~done).any(), f"deactivated {_abi.FAILURE_CRITERIA[i]}: condition never met in a surviving env"
    assert 0 < bin(sc.active_failure_mask).count("1") and (npz["stats"][:, 1] > 0).any() and (npz["stats"][:, 2] > 0).any()
    if blind:
        assert sc.active_failure_mask != (1 << _abi.NUM_FAIL) - 1                # a proper subset
        succ = npz["crit_succ"].astype(bool)[:, 0]
        assert (succ & done).any() and (npz["stats"][:, 0] > 0).any() and (npz["rew"] > 1500).any()
        ts = npz["task_state"]
        assert (ts[:, 0] == 2).any() and (ts[:, 0] == 3).any() and ts[:, 4].any() and ts[:, 5].any()
    b = npz["binaries"]
    assert set(np.unique(b)) == {0.0, 1.0}
    assert (b.reshape(-1, b.shape[2]).min(axis=0) == 0).all() and (b.reshape(-1, b.shape[2]).max(axis=0) == 1).all()
    assert len(json.loads(str(npz["binary_keys"]))) == (4 if blind else 1)
    assert len(npz["snap_step"]) >= 2 and done[npz["snap_step"]].any()            # snapshots include a step with resets


def _disagrees(sc, model, npz):
    """True if an oracle built from `sc` does not reproduce the golden: another action / observation width, a done mismatch,
    or an error above the replay's tolerance in any compared quantity.  (The replay runs with its checks on and stops at the
    first one that fails, so its own tolerances decide; with check=False it would walk on past a done mismatch with the
    golden's reset bookkeeping.)"""
    if int(sc.num_actions) != npz["actions"].shape[2] or int(sc.num_obs) != npz["obs"].shape[2]:
        return "shape"
    try:
        replay(Oracle(sc, model.to_struct()), npz)
    except AssertionError as e:
        return str(e).strip().splitlines()[0][:80] or "assert"
    return None


@pytest.mark.parametrize("name", CFG_SCENARIOS)
def test_every_override_is_live(golden_dir, name):
    """Each key of the scenario's cfg_overrides, put back to its default on its own, must make the oracle's replay disagree
    with the golden.  An override whose revert changes nothing would not be tested by the scenario."""
    from dexrobot_isaac_amd.config import default_cfg
    npz = _load(golden_dir, name)
    over = json.loads(str(npz["cfg_overrides"]))
    dflt = default_cfg(str(npz["task"]))
    assert len(over) >= 6
    sc, model = build_sim_config(scenario_config(npz))
    assert _disagrees(sc, model, npz) is None
    dead = []
    for key in over:
        cfg = scenario_config(npz)
        d = cfg
        parts = key.split(".")
        for p in parts[:-1]:
            d = d[p]
        d[parts[-1]] = _get(dflt, key)
        assert _get(dflt, key) != over[key], key
        sc, model = build_sim_config(cfg)
        if _disagrees(sc, model, npz) is None:
            dead.append(key)
    assert not dead, f"overrides whose revert to the default changes nothing: {dead}"
