"""What the tests of the query kernels share (test_render, test_kindyn, test_ik, test_proximity, test_inverse_dynamics,
test_forward_dynamics): the queries are pure functions of q (and qd) that write caller-owned memory only, so every suite loads the
library, poses cores, stubs the core under DexHandEnv, puts its outputs between guard rows and checks that nothing of the instance
changed in the same way (purity_frame: a suite passes its calls).  A plain module: no fixtures."""
import numpy as np

from dexrobot_isaac_amd.config import build_sim_config, default_cfg

GUARD = -7.0


def load_lib():
    from dexrobot_isaac_amd import _lib
    from dexrobot_isaac_amd.build import build_lib
    build_lib()
    return _lib.load()


def dev(a):
    """None and tensors as they are, arrays as contiguous tensors on the GPU."""
    import torch
    if a is None or torch.is_tensor(a):
        return a
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")


def stub_core(record, **methods):
    """A core factory with just enough of a core for DexHandEnv's own argument checks: method `name` appends record[name](its
    arguments) to `calls` and computes nothing; `methods` are defined as given.  Every core made has a class and a list of its own."""
    def factory(sim_cfg, model_struct, device="cpu"):
        from oracle.py_backend import OracleCore
        rec = {name: (lambda self, *a, _what=what, **kw: self.calls.append(_what(*a, **kw))) for name, what in record.items()}
        return type("Stub", (OracleCore,), dict(calls=[], **rec, **methods))(sim_cfg, model_struct, device)
    return factory


def setup(n, task="BlindGrasping", model=None, free_bodies=False, restore=None):
    """(sc, ms) of n envs, the struct a fresh one for the caller to edit.  model: None for the default hand, "scaled" for
    scaled_model on it, "generic" for the model of tests/generic_model.py, with its free_body_frames if free_bodies and with the
    property `restore` (a name of generic_properties()) put back to the default model's value."""
    if model == "generic":
        from tests import generic_model
        sc, _, ms = generic_model.build(n, task, free_bodies=free_bodies, restore=restore)
        return sc, ms
    assert model in (None, "scaled") and not free_bodies and restore is None
    cfg = default_cfg(task)
    cfg["env"]["numEnvs"] = n
    sc, hand = build_sim_config(cfg)
    ms = hand.to_struct()
    return sc, scaled_model(ms) if model == "scaled" else ms


def generic_hand():
    """The HandModel of tests/generic_model.py, a copy of the caller's own: make_env(..., hand_model=generic_hand())."""
    from tests import generic_model
    return generic_model.build(1)[1]


def generic_properties():
    """The names of the structural properties the generic model lacks (tests/generic_model.py::RESTORE)."""
    from tests import generic_model
    return list(generic_model.RESTORE)


def scaled_model(ms, seed=8):
    """The suites' second model: per-joint scaled offsets, centres of mass and masses, finger links with off-diagonal inertia --
    no constant of the default model is baked in, and the diagonal-inertia shortcut of the step path is not taken.  It keeps every
    zero of the default model a zero; the model without them is tests/generic_model.py.  Changes `ms` in place and returns it."""
    rng = np.random.default_rng(seed)
    for j in range(len(ms.mass)):
        fp, fc, fm = rng.uniform(0.7, 1.4, 3)
        for i in range(3):
            ms.jpoff[j][i] *= fp
            ms.com[j][i] *= fc
        ms.mass[j] *= fm
        if j >= 6:                                                             # [[1, .3, -.2], [.3, 1, .25], [-.2, .25, 1]] is positive definite
            a, b, d = ms.inertia[j][0], ms.inertia[j][1], ms.inertia[j][2]
            ms.inertia[j][3], ms.inertia[j][4], ms.inertia[j][5] = 0.3 * (a * b) ** 0.5, -0.2 * (a * d) ** 0.5, 0.25 * (b * d) ** 0.5
    return ms


def guarded(k, *tail):
    """A NaN-filled (k, *tail) float32 device view between one leading and one trailing guard row."""
    import torch
    full = torch.full((k + 2,) + tail, float("nan"), dtype=torch.float32, device="cuda:0")
    full[0], full[-1] = GUARD, GUARD
    return full, full[1:-1]


def guards_ok(full):
    import torch
    torch.cuda.synchronize()
    assert bool((full[0] == GUARD).all()) and bool((full[-1] == GUARD).all()), "a guard row was written"


def pose_core(core, q, box=None, box_quat=None, qd=None):
    """Pose every env through the API tensors and the indexed setters.  The box: (n, 7) centre + quaternion xyzw, or (n, 3)
    positions with `box_quat` (n, 4); its velocities are zeroed."""
    import torch
    ids = torch.arange(core.N)
    core.dof_state[:, :, 0] = torch.as_tensor(q, device=core.device)
    core.dof_state[:, :, 1] = 0.0 if qd is None else torch.as_tensor(qd, device=core.device)
    core.set_dof_state_indexed(ids)
    if box is not None:
        if box_quat is not None:
            box = np.concatenate([box, box_quat], axis=1)
        core.root_state[:, 1, :7] = torch.as_tensor(box, device=core.device)
        core.root_state[:, 1, 7:] = 0.0
        core.set_root_state_indexed(ids)
    torch.cuda.synchronize()
    assert (core.field("q").t().cpu().numpy() == q).all()
    if box is not None:
        assert (core.field("box_pos").t().cpu().numpy() == box[:, :3]).all() and (core.field("box_quat").t().cpu().numpy() == box[:, 3:]).all()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def snapshot(core):
    """Every tensor of the instance a query could reach, and the step stamp."""
    import torch
    torch.cuda.synchronize()
    names = ("arena", "stats", "counters", "obs_buf", "rew_buf", "reset_buf", "episode_step_count", "episode_length", "dof_state",
             "root_state", "rigid_body_states", "contact_forces_all", "full_dof_targets", "masks")
    snap = {n: getattr(core, n).clone() for n in names}
    snap["stamp"] = core.get_step_stamp()
    return snap


def same(a, b):
    import torch
    return all((a[k] == b[k]) if k == "stamp" else torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) for k in a)


def purity_frame(calls, between=None, n=70, seed=4, steps=(3, 5)):
    """The queries are pure and deterministic: two cores of n BlindGrasping envs, reset and stepped steps[0] times with the same
    seeded actions; on one of them `calls(core)` (a list of host arrays), `between(core)` (the same queries on other rows and
    with other arguments) and `calls(core)` again.  Nothing of the instance changed, the two results are bit-identical, and
    after steps[1] more steps the core equals the twin that never made a call.  Returns the first result for the caller's own
    assertions on it."""
    import torch
    from dexrobot_isaac_amd.core import DexSimCore
    sc, ms = setup(n)
    core, twin = DexSimCore(sc, ms, "cuda:0"), DexSimCore(sc, ms, "cuda:0")
    g = torch.Generator().manual_seed(seed)
    acts = [(2 * torch.rand(n, 18, generator=g) - 1).cuda() for _ in range(sum(steps))]
    for c in (core, twin):
        c.reset()
        for a in acts[:steps[0]]:
            c.step(a)
    before = snapshot(core)
    first = calls(core)
    if between is not None:
        between(core)
    second = calls(core)
    assert same(before, snapshot(core))                                        # nothing of the instance changed
    raw = lambda a: np.ascontiguousarray(a).view(np.uint8)
    assert len(first) == len(second) and all((raw(x) == raw(y)).all() for x, y in zip(first, second))   # two calls on one state: bit-identical
    for a in acts[steps[0]:]:
        core.step(a)
        twin.step(a)
    assert same(snapshot(core), snapshot(twin))                                # ... and the run continues like a twin that never called them
    for c in (core, twin):
        c.close()
    return first
