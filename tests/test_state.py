"""Save, restore and fork of simulation state: dexsim_state_layout / dexsim_save_state / dexsim_load_state / dexsim_copy_envs /
dexsim_{get,set}_step_stamp, DexSimCore.{state_bank, save_state, load_state, copy_envs} and DexHandEnv.{get_state, set_state,
save_states, load_states, fork_envs} with EnvState.

The GPU tests run protocol P, the state of bench.py:training_like at test size: BlindGrasping with the hand translation range
widened to 0.40 m, injected reset samples that put every hand onto its box, de-synchronised episode clocks and 0.2 x random
actions -- hand contacts in every workgroup (general contact path), resets in most steps (second, device-gated physics step)."""
import ctypes as C

import numpy as np
import pytest
import torch

from dexrobot_isaac_amd import _abi, _lib, default_cfg, make_env
from dexrobot_isaac_amd._lib import DexSimError
from dexrobot_isaac_amd.build import build_lib
from dexrobot_isaac_amd.config import build_sim_config
from dexrobot_isaac_amd.env import EnvState

DEV = "cuda:0"
SCRATCH = ["jframe", "ufree", "fac_finv", "fac_g", "cgeom", "ccode", "crow", "crowq", "clam", "chdr", "cstage", "csplit"]
API = ["obs_buf", "rew_buf", "reset_buf", "episode_step_count", "episode_length", "dof_state", "root_state", "full_dof_targets", "masks"]


@pytest.fixture(scope="module")
def lib():
    build_lib()
    return _lib.load()


def _layouts(lib, sc):
    out = []
    for fn in (lib.dexsim_arena_layout, lib.dexsim_state_layout):
        fields = (_abi.DexSimField * 128)()
        nf, words = C.c_int(), C.c_size_t()
        assert fn(C.byref(sc), fields, 128, C.byref(nf), C.byref(words)) == 0
        out.append(([(fields[i].name.decode(), int(fields[i].rows), int(fields[i].is_int), int(fields[i].offset))
                     for i in range(nf.value)], int(words.value)))
    return out


# ---------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("task", ["BlindGrasping", "BaseTask"])
def test_state_layout(lib, task):
    cfg = default_cfg(task)
    cfg["env"]["numEnvs"] = 100
    sc, _ = build_sim_config(cfg)
    (arena, arena_words), (rec, record_words) = _layouts(lib, sc)
    NS = 128
    names = [f[0] for f in rec]
    assert len(set(names)) == len(names)
    pos = 0
    for name, rows, is_int, off in sorted(rec, key=lambda f: f[3]):      # the sections tile [0, record_words) without gaps
        assert off == pos and rows > 0, name
        pos += rows
    assert pos == record_words
    by_name = {f[0]: f for f in arena}
    arena_part = [f for f in rec if not f[0].startswith("api.")]
    for name, rows, is_int, _ in arena_part:
        assert name in by_name and by_name[name][1:3] == (rows, is_int), name
    assert not set(SCRATCH) & set(names) and {"ncontact", "wlam", "wgen", "reset_count", "box_mass", "box_mu"} <= set(names)
    assert set(by_name) - set(SCRATCH) == {f[0] for f in arena_part}      # every arena field is persistent or listed scratch
    assert {n for n in names if n.startswith("api.")} == {"api." + n for n in API}
    assert dict((f[0], f[1]) for f in rec)["api.obs_buf"] == sc.num_obs
    assert record_words < arena_words / NS / 3
    nf, words = C.c_int(), C.c_size_t()
    fields = (_abi.DexSimField * 128)()
    assert lib.dexsim_state_layout(C.byref(sc), fields, 3, C.byref(nf), C.byref(words)) == 5      # DEXSIM_ERR_LAYOUT
    assert lib.dexsim_state_layout(C.byref(sc), None, 0, C.byref(nf), C.byref(words)) == 0 and nf.value == len(rec)
    assert lib.dexsim_state_layout(None, fields, 128, C.byref(nf), C.byref(words)) == 1


def test_state_calls_reject_null_handle_and_bad_k(lib):
    sc, _ = build_sim_config(default_cfg("BaseTask"))
    nf, words, stamp = C.c_int(), C.c_size_t(), C.c_int()
    ERR_ARG = 1
    assert lib.dexsim_state_layout(C.byref(sc), None, 0, None, C.byref(words)) == ERR_ARG
    sc.num_envs = 0
    assert lib.dexsim_state_layout(C.byref(sc), None, 0, C.byref(nf), C.byref(words)) == ERR_ARG
    ids = (C.c_int64 * 4)(0, 1, 2, 3)      # never dereferenced: the argument checks come first
    bank = (C.c_float * 64)()
    for fn in (lib.dexsim_save_state, lib.dexsim_load_state):
        assert fn(None, ids, ids, 4, bank, 64, None) == ERR_ARG and b"null handle" in lib.dexsim_last_error()
        assert fn(None, None, None, 0, bank, 64, None) == ERR_ARG and b"null handle" in lib.dexsim_last_error()
        assert fn(None, ids, ids, -1, bank, 64, None) == ERR_ARG and b"k must not be negative" in lib.dexsim_last_error()
    assert lib.dexsim_copy_envs(None, ids, ids, 4, None) == ERR_ARG and b"null handle" in lib.dexsim_last_error()
    assert lib.dexsim_copy_envs(None, ids, ids, -3, None) == ERR_ARG and b"k must not be negative" in lib.dexsim_last_error()
    assert lib.dexsim_get_step_stamp(None, C.byref(stamp)) == ERR_ARG and b"null handle" in lib.dexsim_last_error()
    assert lib.dexsim_set_step_stamp(None, 5) == ERR_ARG and b"null handle" in lib.dexsim_last_error()


BAD_RANGES = [        # (field: value, ...) on top of the valid ranges, and the field the refusal must name
    ({"dr_mass_lo": 0.0}, "dr_mass_lo"), ({"dr_mass_lo": -0.05}, "dr_mass_lo"), ({"dr_mass_lo": 0.3}, "dr_mass_lo"),
    ({"dr_mu_lo": 2.0}, "dr_mu_lo"), ({"dr_mu_lo": -0.1}, "dr_mu_lo"),
    ({"dr_mass_lo": float("nan")}, "dr_mass_lo"), ({"dr_mass_hi": float("inf")}, "dr_mass_hi"),
    ({"dr_mu_lo": float("nan")}, "dr_mu_lo"), ({"dr_mu_hi": float("inf")}, "dr_mu_hi"), ({"dr_mu_hi": float("nan")}, "dr_mu_hi"),
]


def test_bad_randomisation_ranges_are_refused(lib):
    """With dr_enabled the draw of k_init reaches 1 / box_mass and the friction cones: dexsim_create (before any device work),
    build_sim_config and the oracle's create refuse a mass bound <= 0, a negative friction bound, lo > hi and non-finite bounds, each
    naming the field; a valid range, and a bad one with dr_enabled = 0, pass the argument checks (up to the missing device here)."""
    from oracle.oracle import Oracle
    cfg = default_cfg("BlindGrasping")
    cfg["env"]["numEnvs"] = 4
    good = {"mass": (0.05, 0.2), "friction": (0.5, 1.5), "seed": 4242}
    sc, model = build_sim_config(cfg, dr=good)
    ms = model.to_struct()
    ERR_ARG, ERR_NO_DEVICE = 1, lib.dexsim_create(C.byref(sc), C.byref(ms), 1 << 20, C.byref(C.c_void_p()))
    assert ERR_NO_DEVICE != ERR_ARG and b"dr_" not in lib.dexsim_last_error()      # no such device: past every argument check
    for edit, field in BAD_RANGES:
        bad, _ = build_sim_config(cfg, dr=good)
        for k, v in edit.items():
            setattr(bad, k, v)
        h = C.c_void_p()
        assert lib.dexsim_create(C.byref(bad), C.byref(ms), 1 << 20, C.byref(h)) == ERR_ARG and not h.value, edit
        assert field.encode() in lib.dexsim_last_error(), (edit, lib.dexsim_last_error())
        with pytest.raises(ValueError, match=field):
            Oracle(bad, ms)
        dr = {"mass": (bad.dr_mass_lo, bad.dr_mass_hi), "friction": (bad.dr_mu_lo, bad.dr_mu_hi)}
        with pytest.raises(ValueError, match=field):
            build_sim_config(cfg, dr=dr)
        bad.dr_enabled = 0                                    # the bounds are not read then
        assert lib.dexsim_create(C.byref(bad), C.byref(ms), 1 << 20, C.byref(h)) == ERR_NO_DEVICE
    degenerate, _ = build_sim_config(cfg, dr={"mass": (0.1, 0.1), "friction": (0.0, 0.0)})       # lo == hi, mu = 0: a configuration
    assert lib.dexsim_create(C.byref(degenerate), C.byref(ms), 1 << 20, C.byref(C.c_void_p())) == ERR_NO_DEVICE
    assert Oracle(degenerate, ms).get("box_mass").min() > 0


def _hand_built_state(**kw):
    g = torch.Generator().manual_seed(1)
    d = dict(version=_abi.STATE_VERSION, record_words=7, num_envs=3, config_hash="ab" * 32, capacity=64, stamp=41,
             bank=torch.rand(7 * 64, generator=g), stats=torch.rand(_abi.STAT_WORDS, generator=g),
             counters=torch.arange(_abi.STAT_WORDS, dtype=torch.int32), actions=torch.rand(3, 18, generator=g),
             enabled_post_action_filters=["velocity_clamp", "position_clamp"])
    d.update(kw)
    return EnvState(**d)


def test_env_state_file_round_trip(tmp_path):
    st = _hand_built_state()
    st.bank[5] = float("nan")                                     # bit patterns survive, not just values
    path = str(tmp_path / "state.pt")
    st.save(path)
    raw = torch.load(path, weights_only=True)                     # a plain dict of CPU tensors, ints and strings
    assert isinstance(raw, dict) and all(isinstance(v, (torch.Tensor, int, str, list)) for v in raw.values())
    back = EnvState.load(path, "cpu")
    for k in ("version", "record_words", "num_envs", "config_hash", "capacity", "stamp", "enabled_post_action_filters"):
        assert getattr(back, k) == getattr(st, k), k
    for k in ("bank", "stats", "counters", "actions"):
        a, b = getattr(back, k), getattr(st, k)
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32)), k
    torch.save({"bank": st.bank}, path)
    with pytest.raises(DexSimError, match="not an EnvState file"):
        EnvState.load(path)


def _oracle_env(n=3, core=None):
    from oracle.py_backend import OracleCore
    return make_env("BlindGrasping", n, "cpu", "cpu", 0, _core_factory=core or OracleCore)


def test_state_api_on_oracle_backed_env_raises_clearly():
    env = _oracle_env()
    ids = torch.tensor([0])
    calls = [lambda: env.get_state(), lambda: env.set_state(_hand_built_state()), lambda: env.state_bank(4),
             lambda: env.save_states(None, ids, ids), lambda: env.load_states(None, ids, ids),
             lambda: env.fork_envs(torch.tensor([0]), torch.tensor([1]))]
    for call in calls:
        with pytest.raises(DexSimError, match="needs the HIP engine.*OracleCore"):
            call()


def test_set_state_names_the_mismatching_field(lib):
    from oracle.py_backend import OracleCore

    class StubCore(OracleCore):
        """The oracle stand-in plus the state methods, none of which may be reached: set_state must refuse first."""
        NS = 64

        def state_layout(self):
            (_, _), (rec, words) = _layouts(lib, self.cfg)
            return {f[0]: (f[3], f[1], bool(f[2])) for f in rec}, words

        def _unreachable(self, *a, **k):
            raise AssertionError("set_state went on with a state that does not fit")
        state_bank = save_state = load_state = copy_envs = get_step_stamp = set_step_stamp = _unreachable

    env = _oracle_env(3, StubCore)
    _, words = env._core.state_layout()
    good = dict(record_words=words, num_envs=3, config_hash=env._config_hash())
    for field, bad in (("version", _abi.STATE_VERSION + 1), ("record_words", words + 1), ("num_envs", 4), ("config_hash", "0" * 64)):
        with pytest.raises(DexSimError, match=f"does not fit this env: {field} is"):
            env.set_state(_hand_built_state(**{**good, field: bad}))
    cfg = default_cfg("BlindGrasping")
    cfg["task"]["hand_translation_range"] = 0.4
    other = make_env("BlindGrasping", 3, "cpu", "cpu", 0, _core_factory=StubCore, cfg=cfg)
    assert other._config_hash() != env._config_hash()


# ---------------------------------------------------------------------------------------------------------------- GPU
def _proto_cfg(obs_dict="all"):
    cfg = default_cfg("BlindGrasping")
    cfg["task"]["hand_translation_range"] = 0.40
    cfg["env"]["obsDict"] = obs_dict
    return cfg


def _proto_samples(rng, n):
    u = rng.random((n, 29))
    u[:, 3:5] = 0.5 + 0.05 * (u[:, 3:5] - 0.5)
    u[:, 5] = 0.1725 + 0.01875 * u[:, 5]
    u[:, 6:9] = 0.5 + 0.1 * (u[:, 6:9] - 0.5)
    u[:, 9] *= 0.19
    u[:, 10:] *= 0.57
    return u.astype(np.float32)


def _actions(rng, n):
    return torch.as_tensor((0.2 * (2 * rng.random((n, 18)) - 1)).astype(np.float32), device=DEV)


def _set_clocks(core, k):
    """episode_step <- k, time_in_stage <- k * control_dt for envs 0 .. len(k) - 1"""
    kt = torch.as_tensor(k, device=DEV)
    core.field("episode_step")[0, : len(k)] = kt.to(torch.int32)
    core.field("time_in_stage")[0, : len(k)] = kt.to(torch.float32) * float(core.cfg.control_dt)


DR = {"mass": (0.05, 0.2), "friction": (0.5, 1.5), "seed": 4242}      # a box mass and friction of its own per env (config 5)


def _proto_core(n, seed, dr=None):
    """Protocol P on a bare DexSimCore; returns (core, rng)."""
    from dexrobot_isaac_amd.core import DexSimCore
    cfg = _proto_cfg()
    cfg["env"]["numEnvs"] = n
    sc, model = build_sim_config(cfg, dr=dr)
    core = DexSimCore(sc, model.to_struct(), DEV)
    rng = np.random.default_rng(seed)
    core.set_reset_samples(_proto_samples(rng, n))
    core.reset()
    _set_clocks(core, rng.integers(0, 199, n))
    return core, rng


def _proto_env(n, seed, obs_dict="all", dr=None):
    env = make_env("BlindGrasping", n, DEV, DEV, 0, cfg=_proto_cfg(obs_dict), domain_randomisation=dr)
    rng = np.random.default_rng(seed)
    env._core.set_reset_samples(_proto_samples(rng, n))
    env.reset()
    _set_clocks(env._core, rng.integers(0, 199, n))
    return env, rng


def _state_rows(core):
    """bool (arena rows,) of the persistent ROWS-layout fields, and the (first row, rows) of wlam, in units of arena rows"""
    layout, _ = core.state_layout()
    total = core.arena.numel() // core.NS
    rows = torch.zeros(total, dtype=torch.bool, device=DEV)
    for name in layout:
        if not name.startswith("api.") and name != "wlam":
            off, r, _ = core.fields[name]
            assert off % core.NS == 0
            rows[off // core.NS: off // core.NS + r] = True
    off, r, _ = core.fields["wlam"]
    return rows, (off // core.NS, r)


def _snapshot(core):
    """clones of the whole arena (as int32 words, padded lanes included) and of every API tensor of the record"""
    torch.cuda.synchronize()
    d = {"arena": core._arena_i32.clone()}
    for name in API:
        d[name] = getattr(core, name).clone()
    return d


def _record_of(core, snap):
    """the record part of a snapshot, all lanes: persistent arena rows, wlam, API tensors"""
    rows, (w0, wr) = _state_rows(core)
    a = snap["arena"].view(-1, core.NS)
    return [a[rows], a[w0: w0 + wr]] + [snap[n] for n in API]


def _env_words(core, snap, envs):
    """per-env view of a snapshot: for every listed env its persistent arena words, wlam quads and API rows"""
    rows, (w0, wr) = _state_rows(core)
    a = snap["arena"].view(-1, core.NS)
    e = torch.as_tensor(envs, device=DEV)
    out = [a[rows][:, e].t(), a[w0: w0 + wr].reshape(wr // 4, core.NS, 4)[:, e].permute(1, 0, 2)]
    for n in API:
        out.append(snap[n][:, e].t() if n == "masks" else snap[n][e])
    return out


def _assert_only_envs_changed(core, before, after, envs):
    """every arena word and API element that differs between the two snapshots belongs to one of `envs`; words are mapped to
    their env through the layout: [row][env] everywhere, [quad][env][4] in wlam; scratch fields must not differ at all"""
    rows, (w0, wr) = _state_rows(core)
    NS = core.NS
    e = torch.as_tensor(envs, device=DEV)
    allowed = torch.zeros(core.arena.numel() // NS, NS, dtype=torch.bool, device=DEV)
    lane = torch.zeros(NS, dtype=torch.bool, device=DEV)
    lane[e] = True
    allowed[rows] = lane
    allowed[w0: w0 + wr].view(wr // 4, NS, 4)[:, e, :] = True
    changed = (before["arena"] != after["arena"]).view(-1, NS)
    assert not bool((changed & ~allowed).any())
    for name in SCRATCH:
        off, r, _ = core.fields[name]
        assert not bool(changed[off // NS: off // NS + r].any()), name
    for n in API:
        b, a = before[n], after[n]
        if n == "masks":
            b, a = b.t(), a.t()
        diff = (b != a).reshape(b.shape[0], -1).any(dim=1)
        assert not bool(diff[~lane[: core.N]].any()), n
    return changed


@pytest.mark.gpu
def test_restore_continues_bit_for_bit():
    """A: a full snapshot (bank + stats + counters + stamp) restored into the same instance, and into a fresh one, replays 12
    steps of protocol P (n = 200: padded last workgroup; device Philox resets in the window) with every output, every
    statistic and every word of every record identical."""
    from dexrobot_isaac_amd.core import DexSimCore
    n = 200
    core, rng = _proto_core(n, 3)
    core.set_reset_samples(None)
    for _ in range(13):
        core.step(_actions(rng, n))
    bank = core.state_bank(core.NS)
    core.save_state(bank)
    stats, counters, stamp = core.stats.clone(), core.counters.clone(), core.get_step_stamp()
    acts = [_actions(rng, n) for _ in range(12)]

    def run(c):
        out = []
        for a in acts:
            c.step(a)
            torch.cuda.synchronize()
            out.append([c.stats.clone()] + _record_of(c, _snapshot(c)))
        return out

    def restore(c):
        c.load_state(bank)
        c.stats.copy_(stats)
        c.counters.copy_(counters)
        c.set_step_stamp(stamp)

    ref = run(core)
    hand = [float(r[0][_abi.STAT["MEAN_HAND_CONTACTS"]]) for r in ref]
    resets = sum(float(r[0][_abi.STAT["NUM_RESETS"]]) for r in ref)
    phys = {int(r[0][_abi.STAT["PHYSICS_STEPS"]]) for r in ref}
    print("A: hand contacts/env per step", hand, "resets", resets, "physics steps", phys)
    assert min(hand) >= 0.4 and resets >= 5 and phys == {1, 2}

    for _ in range(5):
        core.step(_actions(rng, n))
    restore(core)
    assert core.get_step_stamp() == stamp
    again = run(core)
    fresh = DexSimCore(core.cfg, core.model, DEV)
    fresh.reset()                                          # one stamp on: the new instance is on the other stamp parity
    assert (fresh.get_step_stamp() ^ stamp) & 1
    restore(fresh)
    third = run(fresh)
    for label, got in (("same instance", again), ("fresh instance", third)):
        for t, (r, g) in enumerate(zip(ref, got)):
            for i, (x, y) in enumerate(zip(r, g)):
                assert x.dtype == y.dtype and torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                                                          y.view(torch.int32) if y.dtype == torch.float32 else y), (label, t, i)


@pytest.mark.gpu
def test_indexed_save_load_touch_exactly_their_envs():
    """B: four envs (first and last lane of the padded last workgroup among them) saved to scattered slots and loaded back 3
    steps later read exactly as at the save, and nothing else in the arena or the API tensors changes across the load."""
    n = 70
    core, rng = _proto_core(n, 3)
    for _ in range(3):
        core.step(_actions(rng, n))
    envs, slots = [69, 3, 64, 0], [5, 0, 2, 7]
    bank = core.state_bank(8)
    core.save_state(bank, env_ids=torch.tensor(envs), slots=torch.tensor(slots))
    first = _snapshot(core)
    for _ in range(3):
        core.step(_actions(rng, n))
    before = _snapshot(core)
    core.load_state(bank, env_ids=torch.tensor(envs), slots=torch.tensor(slots))
    after = _snapshot(core)
    for x, y in zip(_env_words(core, first, envs), _env_words(core, after, envs)):
        assert torch.equal(x, y)
    changed = _assert_only_envs_changed(core, before, after, envs)
    assert int(changed.sum()) > 4 * 100                      # the load did move the envs back
    # the bank holds the records where the layout says: the q rows and the obs_buf rows of the four slots
    assert torch.equal(bank.section("q")[:, slots], first["arena"].view(torch.float32).view(-1, core.NS)[:26][:, envs])
    assert torch.equal(bank.section("api.obs_buf")[:, slots].t(), first["obs_buf"][envs])
    off, r, _ = core.fields["wlam"]
    w = first["arena"].view(torch.float32).view(-1, core.NS)[off // core.NS: off // core.NS + r].reshape(r // 4, core.NS, 4)
    assert torch.equal(bank.section("wlam")[:, slots], w[:, envs].permute(0, 2, 1).reshape(r, 4))
    assert torch.equal(bank.section("api.episode_step_count")[0, slots].to(torch.int64), first["episode_step_count"][envs])
    # bad arguments that need a handle
    with pytest.raises(DexSimError, match="capacity >= NS"):
        core.save_state(bank)                                # identity needs a slot per lane
    rc = core.lib.dexsim_save_state(core.h, None, None, 0, None, 128, None)
    assert rc == 1 and b"bank is NULL" in core.lib.dexsim_last_error()


def _fork_of_a_whole_workgroup(dr):
    n = 128
    from dexrobot_isaac_amd.core import DexSimCore
    cfg = _proto_cfg()
    cfg["env"]["numEnvs"] = n
    sc, model = build_sim_config(cfg, dr=dr)
    core = DexSimCore(sc, model.to_struct(), DEV)
    rng = np.random.default_rng(5)
    u = _proto_samples(rng, 64)
    core.set_reset_samples(np.concatenate([u, u]))
    core.reset()
    _set_clocks(core, rng.integers(0, 199, 64))
    src, dst = torch.arange(64), torch.arange(64, 128)
    if dr:                                                   # every lane's destination holds another box before the fork
        for f in ("box_mass", "box_mu"):
            assert bool((core.field(f)[0, :64] != core.field(f)[0, 64:128]).all()), f
    core.copy_envs(src, dst)
    hand, resets = [], 0
    for t in range(16):
        a = _actions(rng, 64)
        core.step(torch.cat([a, a]))
        snap = _snapshot(core)
        for i, (x, y) in enumerate(zip(_env_words(core, snap, src), _env_words(core, snap, dst))):
            assert torch.equal(x, y), (t, i)
        hand.append(float(core.stats[_abi.STAT["MEAN_HAND_CONTACTS"]]))
        resets += int(core.reset_buf[:64].sum())
    print("C1: hand contacts/env per step", hand, "resets of the sources", resets)
    assert min(hand) >= 0.2 and resets >= 2


@pytest.mark.gpu
def test_fork_of_a_whole_workgroup_continues_bitwise():
    """C1: workgroup 0 copied onto workgroup 1 in lane order, then driven by the same actions and the same injected reset
    samples: env i + 64 equals env i on every record word and API row for 16 steps."""
    _fork_of_a_whole_workgroup(None)


@pytest.mark.gpu
def test_scattered_fork_and_its_precondition():
    """C2: copy_envs with a repeated source across workgroups: destinations equal their sources, nothing else changes;
    fork_envs refuses destinations that repeat or are also sources."""
    n = 200
    env, rng = _proto_env(n, 3)
    core = env._core
    for _ in range(2):
        env.step(_actions(rng, n))
    src, dst = [5, 69, 5], [100, 1, 130]
    before = _snapshot(core)
    env.fork_envs(src, dst)
    after = _snapshot(core)
    for x, y in zip(_env_words(core, before, src), _env_words(core, after, dst)):
        assert torch.equal(x, y)
    changed = _assert_only_envs_changed(core, before, after, dst)
    assert int(changed.sum()) > 3 * 100
    with pytest.raises(DexSimError, match="also a source"):
        env.fork_envs([5, 69], [69, 7])
    with pytest.raises(DexSimError, match="more than once"):
        env.fork_envs([5, 6], [7, 7])
    with pytest.raises(DexSimError, match=r"must be in \[0, 200\)"):
        env.fork_envs([5], [200])
    env.fork_envs([5], [6], check=False)
    assert torch.equal(core.obs_buf[5], core.obs_buf[6])
    _assert_only_envs_changed(core, after, _snapshot(core), [6])


# ------------------------------------------------------------------------------------- the record carries the env's box (include/dexsim.h)
def _box_rows(core, envs=slice(None)):
    torch.cuda.synchronize()
    return torch.stack([core.field("box_mass")[0, envs], core.field("box_mu")[0, envs]]).clone()


@pytest.mark.gpu
def test_fork_of_a_whole_workgroup_takes_the_sources_boxes():
    """C1 with a box mass and friction of its own per env: a copy_envs that left the two rows behind would let every destination
    step on with its own box, and env i + 64 would leave env i in the first sub-step with a contact."""
    _fork_of_a_whole_workgroup(DR)


@pytest.mark.gpu
def test_scattered_fork_takes_the_sources_boxes():
    """C2's scattered fork_envs across workgroups, per-env boxes: the destinations hold their sources' mass and friction (other
    numbers than before), every record word of the source, and nothing else changes."""
    n = 200
    env, rng = _proto_env(n, 3, dr=DR)
    core = env._core
    for _ in range(2):
        env.step(_actions(rng, n))
    src, dst = [5, 69, 5], [100, 1, 130]
    before = _snapshot(core)
    box = _box_rows(core)
    assert bool((box[:, src] != box[:, dst]).all())
    env.fork_envs(src, dst)
    after = _snapshot(core)
    assert torch.equal(_box_rows(core, dst), box[:, src])
    for x, y in zip(_env_words(core, before, src), _env_words(core, after, dst)):
        assert torch.equal(x, y)
    _assert_only_envs_changed(core, before, after, dst)


@pytest.mark.gpu
def test_restore_into_an_instance_with_another_draw_continues_bit_for_bit():
    """A with per-env boxes, n = 130: a full snapshot restored into a fresh instance created with another dr_seed -- whose own boxes
    differ in every env -- replays 12 steps of protocol P like the source, on every statistic and every word of every record."""
    from dexrobot_isaac_amd.core import DexSimCore
    n = 130
    core, rng = _proto_core(n, 3, dr=DR)
    core.set_reset_samples(None)
    for _ in range(5):
        core.step(_actions(rng, n))
    bank = core.state_bank(core.NS)
    core.save_state(bank)
    stats, counters, stamp = core.stats.clone(), core.counters.clone(), core.get_step_stamp()
    box = _box_rows(core)
    acts = [_actions(rng, n) for _ in range(12)]

    def run(c):
        out = []
        for a in acts:
            c.step(a)
            torch.cuda.synchronize()
            out.append([c.stats.clone()] + _record_of(c, _snapshot(c)))
        return out

    ref = run(core)
    assert torch.equal(_box_rows(core), box)                 # (the steps and their resets leave the boxes alone)
    cfg = _proto_cfg()
    cfg["env"]["numEnvs"] = n
    sc, model = build_sim_config(cfg, dr={**DR, "seed": 99})
    fresh = DexSimCore(sc, model.to_struct(), DEV)
    fresh.reset()
    assert bool((_box_rows(fresh) != box).all())
    fresh.load_state(bank)
    fresh.stats.copy_(stats)
    fresh.counters.copy_(counters)
    fresh.set_step_stamp(stamp)
    assert torch.equal(_box_rows(fresh), box)
    for t, (r, g) in enumerate(zip(ref, run(fresh))):
        for i, (x, y) in enumerate(zip(r, g)):
            assert x.dtype == y.dtype and torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                                                      y.view(torch.int32) if y.dtype == torch.float32 else y), (t, i)
    hand = [float(r[0][_abi.STAT["MEAN_HAND_CONTACTS"]]) for r in ref]
    print("per-env boxes: hand contacts/env per step", hand)
    assert min(hand) > 0.0                                   # hands on boxes in every step: mass and friction entered the contact rows


@pytest.mark.gpu
def test_indexed_load_into_other_lanes_brings_the_boxes():
    """B with per-env boxes: four records saved from envs a, loaded into other lanes b (both workgroups, the padded one's first and
    last live lane among them): env b then holds env a's mass and friction and every other record word of a at the save, and nothing
    else changes."""
    n = 70
    core, rng = _proto_core(n, 3, dr=DR)
    for _ in range(3):
        core.step(_actions(rng, n))
    a, slots, b = [69, 3, 64, 0], [5, 0, 2, 7], [1, 68, 65, 40]
    bank = core.state_bank(8)
    core.save_state(bank, env_ids=torch.tensor(a), slots=torch.tensor(slots))
    first, box = _snapshot(core), _box_rows(core)
    assert bool((box[:, a] != box[:, b]).all())
    assert torch.equal(bank.section("box_mass")[0, slots], box[0, a]) and torch.equal(bank.section("box_mu")[0, slots], box[1, a])
    for _ in range(3):
        core.step(_actions(rng, n))
    before = _snapshot(core)
    core.load_state(bank, env_ids=torch.tensor(b), slots=torch.tensor(slots))
    after = _snapshot(core)
    assert torch.equal(_box_rows(core, b), box[:, a])
    for x, y in zip(_env_words(core, first, a), _env_words(core, after, b)):
        assert torch.equal(x, y)
    _assert_only_envs_changed(core, before, after, b)


def _same(a, b, path="extras"):
    if isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            _same(a[k], b[k], f"{path}.{k}")
    else:
        assert torch.equal(a, b), path


@pytest.mark.gpu
@pytest.mark.parametrize("obs_dict", ["all", "policy"])
def test_env_get_state_set_state(obs_dict, tmp_path):
    """D: a twin interrupted by get_state / 4 foreign steps / set_state stays equal to its undisturbed twin; a fresh env that
    loads the same state from a file does too; at set_state the env-owned views read as at get_state, in place."""
    n = 128
    env_a, rng = _proto_env(n, 7, obs_dict)
    env_b, _ = _proto_env(n, 7, obs_dict)
    for e in (env_a, env_b):
        e._core.set_reset_samples(None)
    for _ in range(5):
        a = _actions(rng, n)
        env_a.step(a)
        env_b.step(a)
    views = {"obs": env_b.obs_buf, "rew": env_b.rew_buf, "done": env_b.reset_buf, "dof": env_b.dof_state,
             "root": env_b.actor_root_state_tensor, "extras": env_b.extras, "obs_dict": env_b.obs_dict}
    state = env_b.get_state()
    assert (state.version, state.num_envs, state.capacity) == (_abi.STATE_VERSION, n, 128)
    kept = {"obs": env_b.obs_buf.clone(), "obs_dict": {k: v.clone() for k, v in env_b.obs_dict.items()},
            "rc": {k: v.clone() for k, v in env_b.extras["reward_components"].items()}, "actions": env_b.actions.clone()}
    path = str(tmp_path / "env_state.pt")
    state.save(path)
    for _ in range(4):
        env_b.step(_actions(rng, n))
    assert not torch.equal(env_b.obs_buf, kept["obs"])
    env_b.set_state(state)
    env_c = make_env("BlindGrasping", n, DEV, DEV, 0, cfg=_proto_cfg(obs_dict))
    env_c.set_state(EnvState.load(path, DEV))
    for e in (env_b, env_c):
        assert torch.equal(e.obs_buf, kept["obs"]) and torch.equal(e.actions, kept["actions"])
        _same(dict(e.obs_dict), kept["obs_dict"], "obs_dict")
        _same(e.extras["reward_components"], kept["rc"], "reward_components")
    for k, v in views.items():                                   # the same tensors, not rebound ones
        now = {"obs": env_b.obs_buf, "rew": env_b.rew_buf, "done": env_b.reset_buf, "dof": env_b.dof_state,
               "root": env_b.actor_root_state_tensor, "extras": env_b.extras, "obs_dict": env_b.obs_dict}[k]
        assert now is v, k
    resets = 0
    for t in range(8):
        a = _actions(rng, n)
        oa, ra, da, xa = env_a.step(a)
        for e in (env_b, env_c):
            o, r, d, x = e.step(a)
            assert torch.equal(o, oa) and torch.equal(r, ra) and torch.equal(d, da), t
            _same(x, xa)
        resets += int(da.sum())
    print("D: resets in the 8 compared steps", resets)
    with pytest.raises(DexSimError, match="num_envs is 128, expected 64"):
        make_env("BlindGrasping", 64, DEV, DEV, 0, cfg=_proto_cfg(obs_dict)).set_state(state)
