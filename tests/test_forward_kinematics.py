"""Forward kinematics on the device (dexsim_forward_kinematics: body states, site poses, centroid) against tests/fk_ref.py, a
float64 reference that shares no code with the engine, and against what the engine itself publishes.

Bounds (GPU against float64 on the same float32-rounded inputs; fk_ref holds the numbers):
  * positions of bodies, sites and the centre of mass: 1e-5 m absolute -- the derivation of tests/test_kindyn.py: sincos_joint is
    good to 2e-7 per half-angle, so a rotation-matrix entry is off by <~ 6e-7 per revolute joint, there are 7 revolute joints from
    the base to a fingertip and levers are below 0.4 m; plus a few spacings of a world coordinate below 2.5 m.  A wrong index, sign
    or offset is >= 1e-3.
  * quaternions: 1e-5 per component, up to a common sign; unit norm to 1e-5.
  * linear and angular velocities, velocity of the centre of mass: 2e-5 x sum |qd| of the row, the bound
    test_kindyn.test_contract_with_published_body_states uses for the same quantities.
  * hand-frame poses: the same.
  * potential energy: M_tot |g| 1e-5, which follows from the bound of the centre of mass.
  * kinetic energy: 2e-5 relative -- ten-joint chains at 6e-7 per joint on the link velocities, squared.
test_reference_identities_and_roundoff measures the reference's own float32 roundoff, the figure these are read against:
e_p = 2.5e-7 m (body origins, |p| <= 1.6 m), 3.7e-7 m (centre of mass), 2.3e-7 (its velocity), 3.8e-7 relative (kinetic) and
2.2e-7 relative (potential) over the 70 poses of seed 21 with rates uniform in +-1.
Every GPU test uses N = 70: two workgroups, six live lanes in the second.  Every device output sits between two guard rows that
must come back untouched.  The rows: poses over the full joint range, rates uniform in +-1; in the last 20 rows the six base rates
are zero and the finger rates +-1, so that the energy terms show the links' rotation.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from dexrobot_isaac_amd import _abi
from dexrobot_isaac_amd.hand_model import BODY_NAMES, HAND_BASE_BODY_NAME
from tests import fk_ref as fr
from tests import kindyn_ref as kr
from tests.query_rig import bits, guarded, guards_ok, load_lib, pose_core, purity_frame, setup, stub_core

N = 70
NB, NJ, NS = _abi.NUM_HAND_BODIES, _abi.NJ, _abi.NSITE


# ------------------------------------------------------------------------------------------------- CPU
@pytest.fixture(scope="module")
def lib():
    return load_lib()


def test_abi_exports_and_null_handle(lib):
    """include/dexsim_fk.h, the part of the header the entry point is declared in, against _abi.FK_PROTOTYPES and the built library,
    as tests/test_abi.py holds include/dexsim.h against _abi.PROTOTYPES: the same names, the same number of parameters."""
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    hdr = open(os.path.join(inc, "dexsim_fk.h")).read()
    assert '#include "dexsim_fk.h"' in open(os.path.join(inc, "dexsim.h")).read()
    assert set(re.findall(r"\b(dexsim_[a-z_]+)\s*\(", hdr)) == set(_abi.FK_PROTOTYPES) == {"dexsim_forward_kinematics"}
    declared = re.findall(r"\b(dexsim_[a-z_]+)\s*\(([^()]*)\)\s*;", hdr)
    assert [name for name, _ in declared] == list(_abi.FK_PROTOTYPES)
    for name, params in declared:
        assert len(params.split(",")) == len(_abi.FK_PROTOTYPES[name]), name
    assert not set(_abi.FK_PROTOTYPES) & set(_abi.PROTOTYPES)
    assert hasattr(lib, "dexsim_forward_kinematics"), "libdexsim.so does not export dexsim_forward_kinematics"
    assert lib.dexsim_forward_kinematics.argtypes == _abi.FK_PROTOTYPES["dexsim_forward_kinematics"]
    assert lib.dexsim_forward_kinematics(None, None, 1, None, None, None, NB, 0, None, None, None, None) == 1     # DEXSIM_ERR_ARG
    assert b"null handle" in lib.dexsim_last_error()


def test_reference_quaternions():
    rng = np.random.default_rng(0)
    q = rng.normal(size=(200, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    R = np.stack([fr.rr.quat_to_mat(x) for x in q])
    assert fr.quat_err(fr.mat_to_quat(R), q).max() <= 1e-14
    a, b = q[:100], q[100:]
    Rab = np.stack([fr.rr.quat_to_mat(x) for x in a]) @ np.stack([fr.rr.quat_to_mat(x) for x in b])
    assert fr.quat_err(fr.qmul(a, b), fr.mat_to_quat(Rab)).max() <= 1e-14
    assert np.abs(fr.qmul(fr.qconj(a), a) - [0, 0, 0, 1]).max() <= 1e-14


def test_reference_identities_and_roundoff():
    """The centroid reference against the fp64 oracle -- 1/2 qd^T M qd and g(q) . qd = -M_tot g . v_C -- and the reference's own
    float32 roundoff, the figures the GPU bounds are read against."""
    _identities_and_roundoff(None)


def test_reference_identities_and_roundoff_generic_model():
    """The same identities and roundoff bars on the model of tests/generic_model.py, every body on a frame of its own."""
    _identities_and_roundoff("generic")


def _identities_and_roundoff(model):
    sc, ms = setup(1, model=model, free_bodies=model is not None)
    fk = fr.HandFK(ms, sc)
    q, qd = fk.test_rows(N, seed=21)
    qd = np.random.default_rng(1021).uniform(-1, 1, (N, NJ)).astype(np.float32)        # every rate uniform in +-1 for these figures
    cen = fk.centroid(q, qd)
    _, o64 = kr.oracle_pair(sc, ms)
    M64, g64 = kr.mass_gravity(o64, q)
    v = qd.astype(np.float64)
    ke = 0.5 * np.einsum("ni,nij,nj->n", v, M64, v)
    e_ke = float((np.abs(cen[:, 7] - ke) / ke).max())
    power = -fk.total_mass * (cen[:, 4:7] @ fk.gravity)
    e_pw = float((np.abs((g64 * v).sum(1) - power) / np.abs(g64 * v).sum(1)).max())
    print(f"centroid reference against the fp64 oracle: kinetic energy {e_ke:.3g} relative, gravity power {e_pw:.3g} relative")
    assert e_ke <= 1e-7 and e_pw <= 1e-7           # two float64 evaluations of the model's float32 constants; a modelling error is >= 1e-3
    b64, b32 = fk.body_states(q, qd), fk.body_states(q, qd, np.float32)
    c32 = fk.centroid(q, qd, np.float32).astype(np.float64)
    s64, s32 = fk.site_poses(q), fk.site_poses(q, dtype=np.float32)
    figs = {"body origins (m)": np.abs(b32[..., 0:3] - b64[..., 0:3]).max(), "|p| max (m)": np.abs(b64[..., 0:3]).max(),
            "body quaternions": fr.quat_err(b32[..., 3:7], b64[..., 3:7]).max(),
            "body twists": np.abs(b32[..., 7:13] - b64[..., 7:13]).max(),
            "site positions (m)": np.abs(s32[..., 0:3] - s64[..., 0:3]).max(),
            "centre of mass (m)": np.abs(c32[:, 0:3] - cen[:, 0:3]).max(), "its velocity": np.abs(c32[:, 4:7] - cen[:, 4:7]).max(),
            "kinetic (relative)": (np.abs(c32[:, 7] - cen[:, 7]) / cen[:, 7]).max(),
            "potential (relative)": (np.abs(c32[:, 3] - cen[:, 3]) / np.abs(cen[:, 3])).max()}
    print("float32 roundoff of the reference: " + ", ".join(f"{k} {float(x):.3g}" for k, x in figs.items()))
    assert figs["body origins (m)"] <= 0.1 * fr.POS_TOL and figs["centre of mass (m)"] <= 0.1 * fr.POS_TOL
    assert figs["kinetic (relative)"] <= 0.1 * fr.KE_TOL


def test_reference_discrimination():
    """Each deliberate mistake of fk_ref.VARIANTS misses the bound of the quantity it spoils by at least 10 x on the tests' own rows."""
    sc, ms = setup(1)
    fk = fr.HandFK(ms, sc)
    q, qd = fk.test_rows(N, seed=21)
    b, c = fk.body_states(q, qd), fk.centroid(q, qd)
    sw, sh = fk.site_poses(q), fk.site_poses(q, hand_frame=True)

    def miss(errors, name):
        e, bound = errors[name]
        return float((e / bound).max())
    cen = lambda v: fr.centroid_errors(fk.centroid(q, qd, variant=v), c, qd, fk.total_mass, fk.gravity)
    found = {
        "no_rotational_energy": miss(cen("no_rotational_energy"), "kinetic energy"),
        "finger_link_massless": min(miss(cen("finger_link_massless"), n) for n in ("centre of mass", "kinetic energy", "potential energy")),
        "centres_at_joint_origins": min(miss(cen("centres_at_joint_origins"), n) for n in ("centre of mass", "kinetic energy")),
        "no_body_q": miss(fr.body_errors(fk.body_states(q, qd, variant="no_body_q"), b, qd), "body quaternion"),
        "no_site_q": min(miss(fr.site_errors(fk.site_poses(q, variant="no_site_q"), sw), "site quaternion"),
                         miss(fr.site_errors(fk.site_poses(q, hand_frame=True, variant="no_site_q"), sh), "site position")),
        "hand_frame_not_conjugated": min(miss(fr.site_errors(fk.site_poses(q, hand_frame=True, variant="hand_frame_not_conjugated"), sh), n)
                                         for n in ("site position", "site quaternion")),
    }
    print("variants miss their bound by: " + ", ".join(f"{k} {v:.3g} x" for k, v in found.items()))
    assert set(found) == set(fr.VARIANTS) and all(v >= 10 for v in found.values())
    # on the rows with a still base the rotational energy is what the finger links have: it shows on every one of them
    e, bound = cen("no_rotational_energy")["kinetic energy"]
    assert (e[N - 20:] >= 10 * bound[N - 20:]).all()


_stub_core = stub_core(dict(
    forward_kinematics=lambda body_states=None, site_poses=None, centroid=None, env_ids=None, q=None, qd=None, bodies=None, hand_frame=False:
        ("fk", *(None if t is None else tuple(t.shape) for t in (body_states, site_poses, centroid, q, qd)), bodies, hand_frame)))


def test_env_argument_validation():
    import torch
    from dexrobot_isaac_amd import make_env
    from oracle.py_backend import OracleCore
    env = make_env("BaseTask", 3, "cpu", "cpu", 0, _core_factory=_stub_core)
    with pytest.raises(ValueError, match="unknown body"):
        env.get_body_states(bodies=["r_f_link9_tip"])
    with pytest.raises(ValueError, match="body index"):
        env.get_body_states(bodies=[NB])
    with pytest.raises(ValueError, match="shape"):
        env.get_body_states(q=torch.zeros(4, NJ - 1))
    with pytest.raises(ValueError, match="qd"):
        env.get_body_states(qd=torch.zeros(3, NJ))                             # a qd override without a q override
    with pytest.raises(ValueError, match="qd"):
        env.get_centroid(q=torch.zeros(4, NJ), qd=torch.zeros(3, NJ))
    with pytest.raises(ValueError, match="sites"):
        env.get_site_poses(sites="fingers")
    with pytest.raises(ValueError, match="frame"):
        env.get_site_poses(frame="palm")
    with pytest.raises(ValueError, match="out"):
        env.get_site_poses("tips", out=torch.zeros(3, 5, 7))                   # out is the full (k, 11, 7) tensor
    with pytest.raises(ValueError, match="out"):
        env.get_centroid(out=torch.zeros(3, 7))
    with pytest.raises(ValueError, match="empty"):
        env.get_site_poses(env_ids=[])
    assert not env._core.calls                                                 # nothing reached the core
    assert env.get_body_states(bodies=["r_f_link2_tip", 6]).shape == (3, 2, 13)
    assert env._core.calls[-1] == ("fk", (3, 2, 13), None, None, None, None, [18, 6], False)
    for sites, ns in (("all", 11), ("base", 1), ("tips", 5), ("pads", 5)):
        assert env.get_site_poses(sites, "hand", q=torch.zeros(5, NJ)).shape == (5, ns, 7)
        assert env._core.calls[-1] == ("fk", None, (5, NS, 7), None, (5, NJ), None, None, True)
    cen = env.get_centroid(q=torch.zeros(4, NJ), qd=torch.zeros(4, NJ))
    assert env._core.calls[-1] == ("fk", None, None, (4, 8), (4, NJ), (4, NJ), None, False)
    assert cen["com"].shape == (4, 3) and cen["com_vel"].shape == (4, 3) and cen["kinetic"].shape == (4,) and cen["potential"].shape == (4,)
    assert all(cen[k].data_ptr() >= cen["data"].data_ptr() and cen[k]._base is cen["data"] for k in ("com", "com_vel", "kinetic", "potential"))
    plain = make_env("BaseTask", 2, "cpu", "cpu", 0, _core_factory=OracleCore)  # the CPU stand-in has no forward kinematics
    for call in (plain.get_body_states, plain.get_site_poses, plain.get_centroid):
        with pytest.raises(NotImplementedError):
            call()


# ------------------------------------------------------------------------------------------------- GPU helpers
gpu_fk = fr.gpu_fk


def _case(ms, sc, seed):
    """A core of N envs posed at the tests' rows and, computed once, every reference the tests share."""
    from dexrobot_isaac_amd.core import DexSimCore
    fk = fr.HandFK(ms, sc)
    core = DexSimCore(sc, ms, "cuda:0")
    core.reset()
    q, qd = fk.test_rows(N, seed)
    pose_core(core, q, qd=qd)
    return dict(core=core, fk=fk, q=q, qd=qd, sc=sc, B64=fk.body_states(q, qd), S64=fk.site_poses(q), H64=fk.site_poses(q, hand_frame=True),
                C64=fk.centroid(q, qd))


def check_all(c, body, site, hand, cen, what, ref=None, qd="case"):
    r = ref or c
    qd = c["qd"] if isinstance(qd, str) else qd
    fk = c["fk"]
    for x in (body, site, hand, cen):
        assert not np.isnan(x).any(), f"{what}: an element was not written"
    fr.check(fr.body_errors(body, r["B64"], qd), what)
    fr.check(fr.site_errors(site, r["S64"], "world-frame site"), what)
    fr.check(fr.site_errors(hand, r["H64"], "hand-frame site"), what)
    fr.check(fr.centroid_errors(cen, r["C64"], qd, fk.total_mass, fk.gravity), what)
    assert (bits(body[:, 0, 7:13]) == 0).all()                                 # hand_mount: a twist of exact +0.0f
    if tuple(c["core"].model.spawn_quat) == (0.0, 0.0, 0.0, 1.0):              # hand_mount under an identity spawn frame: one exact sum
        spawn = np.array(list(c["core"].model.spawn_pos), dtype=np.float32)      # (a turned spawn frame: the body position bound above)
        assert (body[:, 0, 0:3] == spawn + np.array(np.ctypeslib.as_array(c["core"].model.body_p), dtype=np.float32)[0]).all()


@pytest.fixture(scope="module")
def posed():
    sc, ms = setup(N)
    c = _case(ms, sc, seed=21)
    c["body"], c["site"], c["cen"] = gpu_fk(c["core"], N)
    _, c["hand"], _ = gpu_fk(c["core"], N, hand_frame=True, want=("site",))
    return c


# ------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_against_float64_reference(posed):
    c = posed
    check_all(c, c["body"], c["site"], c["hand"], c["cen"], "default model")
    assert np.abs(c["hand"][:, 0] - [0, 0, 0, 0, 0, 0, 1]).max() <= 1e-6       # site 0 in its own frame


@pytest.mark.gpu
def test_different_model():
    """The scaled model of test_kindyn.test_different_model: per-joint scaled offsets, centres of mass and masses, finger links with
    off-diagonal inertia -- no constant of the default model is baked in."""
    sc, ms = setup(N, model="scaled")
    c = _case(ms, sc, seed=22)
    body, site, cen = gpu_fk(c["core"], N)
    _, hand, _ = gpu_fk(c["core"], N, hand_frame=True, want=("site",))
    check_all(c, body, site, hand, cen, "scaled model")
    c["core"].close()


@pytest.mark.gpu
def test_structure_free_model():
    """The model of tests/generic_model.py, which has none of the default model's exact zeros, ones and repeated numbers, every body
    on a frame of its own: bodies, world- and hand-frame sites and the centroid against the float64 reference, and the contract
    with what the engine publishes (publish_body) and with the Jacobian, the mass matrix and the gravity force on this model."""
    sc, ms = setup(N, model="generic", free_bodies=True)
    c = _case(ms, sc, seed=23)
    c["body"], c["site"], c["cen"] = gpu_fk(c["core"], N)
    _, c["hand"], _ = gpu_fk(c["core"], N, hand_frame=True, want=("site",))
    check_all(c, c["body"], c["site"], c["hand"], c["cen"], "generic model")
    assert np.abs(c["hand"][:, 0] - [0, 0, 0, 0, 0, 0, 1]).max() <= 1e-6       # site 0 in its own frame
    _contract_with_published_state(c)
    c["core"].close()


@pytest.mark.gpu
def test_contract_with_published_state(posed):
    """What the engine publishes for the same state -- rigid_body_states, the arena's site_pose and hand_vel -- and what the other
    queries say about it: J qd, 1/2 qd^T M qd, g . qd."""
    _contract_with_published_state(posed)


def _contract_with_published_state(c):
    import torch
    core, q, qd, fk = c["core"], c["q"], c["qd"], c["fk"]
    pose_core(core, q, qd=qd)
    core.refresh_body_states()
    torch.cuda.synchronize()
    body, site, cen = gpu_fk(core, N)
    assert (bits(body) == bits(c["body"])).all() and (bits(site) == bits(c["site"])).all() and (bits(cen) == bits(c["cen"])).all()
    rbs = core.rigid_body_states[:, :NB].cpu().numpy()
    fr.check(fr.body_errors(body, rbs, qd), "against rigid_body_states")
    arena_sites = core.field("site_pose").t().cpu().numpy().reshape(N, NS, 7)
    fr.check(fr.site_errors(site, arena_sites, "world-frame site"), "against the arena's site_pose")
    hb = BODY_NAMES.index(HAND_BASE_BODY_NAME)
    w = body[:, hb, 10:13].astype(np.float64)
    v0 = body[:, hb, 7:10] + np.cross(w, site[:, 0, 0:3].astype(np.float64) - body[:, hb, 0:3])     # the twist at site 0
    hand_vel = core.field("hand_vel").t().cpu().numpy().astype(np.float64)
    err = np.abs(np.concatenate([v0, w], 1) - hand_vel).max(1)
    bound = fr.VEL_TOL * np.abs(qd).sum(1)
    print(f"site 0's twist against the arena's hand_vel: max error {err.max():.3g}, smallest bound {bound.min():.3g}")
    assert (err <= bound).all()
    # the other queries at the same state
    full, jac = guarded(N, NB, 6, NJ)
    core.body_jacobian(jac)
    guards_ok(full)
    twist = np.einsum("nbdj,nj->nbd", jac.cpu().numpy().astype(np.float64), qd.astype(np.float64))
    err = np.abs(twist - body[:, :, 7:13]).max(axis=(1, 2))
    print(f"jac @ qd against body_states[:, :, 7:13]: max error {err.max():.3g}, smallest bound {bound.min():.3g}")
    assert (err <= bound).all()
    M, g = kr.gpu_mass(core, N)
    v = qd.astype(np.float64)
    ke = 0.5 * np.einsum("ni,nij,nj->n", v, M.astype(np.float64), v)
    # 1/2 qd^T M qd from the device's M: its entries are good to 4 e_M sqrt(M_ii M_jj) (tests/test_kindyn.py), so the form is good
    # to 4 e_M (sum_i sqrt(M_ii) |qd_i|)^2 / 2; e_M from the fp32 oracle on these poses as there
    o32, o64 = kr.oracle_pair(c["sc"], core.model)
    M32, g32 = kr.mass_gravity(o32, q)
    M64, g64 = kr.mass_gravity(o64, q)
    e_M, e_g = kr.err_M(M32, M64), kr.err_g(g32, g64, M64)
    d = np.sqrt(np.einsum("nii->ni", M64))
    b_ke = fr.KE_TOL * ke + 0.5 * 4 * e_M * ((d * np.abs(v)).sum(1)) ** 2
    err = np.abs(cen[:, 7] - ke)
    print(f"kinetic against 1/2 qd^T M qd of the device: max error {err.max():.3g}, max relative {(err / ke).max():.3g}, smallest bound {b_ke.min():.3g}")
    assert (err <= b_ke).all()
    # g . qd = -M_tot g . v_C: the gravity force is good to 4 e_g max_j |g_j| / sqrt(M_jj) per sqrt(M_jj) (err_g), the velocity of the
    # centre of mass to VEL_TOL sum |qd|
    power = (g.astype(np.float64) * v).sum(1)
    b_pw = 4 * e_g * (np.abs(g64) / d).max(1) * (d * np.abs(v)).sum(1) + fk.total_mass * np.linalg.norm(fk.gravity) * bound
    err = np.abs(power + fk.total_mass * (cen[:, 4:7].astype(np.float64) @ fk.gravity))
    print(f"gravity . qd against -M_tot g . com_vel: max error {err.max():.3g}, smallest bound {b_pw.min():.3g}")
    assert (err <= b_pw).all()


@pytest.mark.gpu
def test_contract_with_observations_and_ik():
    """Hand-frame tips and pads against the observation stage after a reset, and the composition IK -> FK: the tips of the
    joint positions solve_fingertip_ik returns are where its residual says."""
    import torch
    from dexrobot_isaac_amd import make_env
    from tests import ik_ref
    env = make_env("BlindGrasping", N, "cuda:0", "cuda:0", 0)
    env.reset()
    for sites, key in (("tips", "fingertip_poses_hand"), ("pads", "fingerpad_poses_hand")):
        mine = env.get_site_poses(sites, frame="hand").cpu().numpy()
        obs = env.obs_dict[key].cpu().numpy().reshape(N, 5, 7)
        fr.check(fr.site_errors(mine, obs, f"hand-frame {sites}"), f"against obs_dict['{key}']")
    world = env.get_site_poses("tips").cpu().numpy()
    fr.check(fr.site_errors(world, env.obs_dict["fingertip_poses_world"].cpu().numpy().reshape(N, 5, 7), "world-frame tips"),
             "against obs_dict['fingertip_poses_world']")
    hik = ik_ref.HandIK(env._model_struct, env._sim_cfg)
    for sites in ("tips", "pads"):
        _, q0, tg = hik.test_poses(N, seed=31, sites=0 if sites == "tips" else 1)
        tg = torch.as_tensor(tg, device="cuda:0")
        _, info = env.solve_fingertip_ik(tg, q=torch.as_tensor(q0, device="cuda:0"), sites=sites, return_info=True)
        tips = env.get_site_poses(sites, q=info["q"])
        dist = (tg - tips[..., 0:3]).double().norm(dim=2)
        err = float((dist - info["residual"].double()).abs().max())
        print(f"IK -> FK ({sites}): | |target - site| - residual | max {err:.3g} m; largest residual {float(info['residual'].max()):.3g} m")
        assert err <= 1e-5
    env.close()


@pytest.mark.gpu
def test_addressing(posed):
    import torch
    c = posed
    core, q, qd, fk = c["core"], c["q"], c["qd"], c["fk"]
    pose_core(core, q, qd=qd)
    ids = [69, 0, 64, 3, 63]                                                   # out of order, across both workgroups
    body, site, cen = gpu_fk(core, len(ids), env_ids=ids)
    assert (bits(body) == bits(c["body"][ids])).all() and (bits(site) == bits(c["site"][ids])).all() and (bits(cen) == bits(c["cen"][ids])).all()
    b1, s1, c1 = gpu_fk(core, 1, env_ids=[37])                                 # k = 1
    assert (bits(b1) == bits(c["body"][[37]])).all() and (bits(s1) == bits(c["site"][[37]])).all() and (bits(c1) == bits(c["cen"][[37]])).all()
    sel = [36, 6, 12]                                                          # out of order
    assert (bits(gpu_fk(core, N, bodies=sel, want=("body",))[0]) == bits(c["body"][:, sel])).all()
    assert (bits(gpu_fk(core, len(ids), env_ids=ids, bodies=sel, want=("body",))[0]) == bits(c["body"][ids][:, sel])).all()
    # each output alone has the bits it has in the combined call
    assert (bits(gpu_fk(core, N, want=("body",))[0]) == bits(c["body"])).all()
    assert (bits(gpu_fk(core, N, want=("site",))[1]) == bits(c["site"])).all()
    assert (bits(gpu_fk(core, N, want=("cen",))[2]) == bits(c["cen"])).all()
    assert (bits(gpu_fk(core, N, hand_frame=True)[1]) == bits(c["hand"])).all()
    # q and qd overrides, k = 130 (three workgroups): rows copied from env state are the state path's bits, the rest meet the reference
    extra, extra_d = fk.test_rows(130 - N, seed=23, still_base=10)
    qo, vo = np.concatenate([q[:40], extra, q[40:]]), np.concatenate([qd[:40], extra_d, qd[40:]])
    src = np.concatenate([np.arange(40), np.full(len(extra), -1), np.arange(40, N)])
    qt, vt = torch.as_tensor(qo, device=core.device), torch.as_tensor(vo, device=core.device)
    bo, so, co = gpu_fk(core, 130, q=qt, qd=vt, env_ids=[-1])                  # env_ids is ignored with an override
    _, ho, _ = gpu_fk(core, 130, q=qt, hand_frame=True, want=("site",))
    st = src >= 0
    assert (bits(bo[st]) == bits(c["body"][src[st]])).all() and (bits(so[st]) == bits(c["site"][src[st]])).all()
    assert (bits(co[st]) == bits(c["cen"][src[st]])).all() and (bits(ho[st]) == bits(c["hand"][src[st]])).all()
    ref = dict(B64=fk.body_states(extra, extra_d), S64=fk.site_poses(extra), H64=fk.site_poses(extra, hand_frame=True),
               C64=fk.centroid(extra, extra_d))
    check_all(c, bo[~st], so[~st], ho[~st], co[~st], "q and qd override", ref=ref, qd=extra_d)
    # qd = None with an override: the poses keep their bits, every velocity word and the kinetic energy are +0.0f
    bz, sz, cz = gpu_fk(core, 130, q=qt)
    assert (bits(bz[..., 0:7]) == bits(bo[..., 0:7])).all() and (bits(sz) == bits(so)).all() and (bits(cz[:, 0:4]) == bits(co[:, 0:4])).all()
    assert (bits(bz[..., 7:13]) == 0).all() and (bits(cz[:, 4:8]) == 0).all()
    # ids outside [0, N) leave their rows as they are
    bad = [5, -1, N, 69]
    bb, sb, cb = gpu_fk(core, 4, env_ids=bad, bodies=sel)
    assert np.isnan(bb[1:3]).all() and np.isnan(sb[1:3]).all() and np.isnan(cb[1:3]).all()
    assert (bits(bb[[0, 3]]) == bits(c["body"][[5, 69]][:, sel])).all() and (bits(sb[[0, 3]]) == bits(c["site"][[5, 69]])).all()
    assert (bits(cb[[0, 3]]) == bits(c["cen"][[5, 69]])).all()
    # argument errors come back as DEXSIM_ERR_ARG, before any launch
    lib, h = core.lib, core.h
    ob, os_, oc = torch.zeros(N, NB, 13, device=core.device), torch.zeros(N, NS, 7, device=core.device), torch.zeros(N + 1, 8, device=core.device)
    pb, ps, pc = (C.c_void_p(t.data_ptr()) for t in (ob, os_, oc))
    pq = C.c_void_p(qt.data_ptr())
    call = lib.dexsim_forward_kinematics
    assert call(h, None, 0, None, None, None, NB, 0, pb, ps, pc, None) == 1                      # k <= 0
    assert call(h, None, N - 1, None, None, None, NB, 0, pb, ps, pc, None) == 1                  # all envs needs k == num_envs
    assert call(h, None, N, None, pq, None, NB, 0, pb, ps, pc, None) == 1                        # qd without q
    assert b"qd" in lib.dexsim_last_error()
    assert call(h, None, N, None, None, None, NB, 0, None, None, None, None) == 1                # all three outputs NULL
    assert b"at least one" in lib.dexsim_last_error()
    assert call(h, None, N, None, None, None, NB - 1, 0, pb, ps, pc, None) == 1                  # all bodies needs nb == 37
    assert call(h, None, N, None, None, (C.c_int * 2)(3, NB), 2, 0, pb, ps, pc, None) == 1       # a body index out of range
    assert call(h, None, N, None, None, (C.c_int * 1)(3), 0, 0, pb, ps, pc, None) == 1           # nb < 1
    assert call(h, None, N, None, None, None, NB, 2, pb, ps, pc, None) == 1                      # an unknown flag bit
    assert b"flag" in lib.dexsim_last_error()
    assert call(h, None, N, None, None, None, NB, 0, C.c_void_p(ob.data_ptr() + 2), ps, pc, None) == 1      # misaligned outputs
    assert call(h, None, N, None, None, None, NB, 0, pb, C.c_void_p(os_.data_ptr() + 2), pc, None) == 1
    assert call(h, None, N, None, None, None, NB, 0, pb, ps, C.c_void_p(oc.data_ptr() + 8), None) == 1
    assert b"aligned" in lib.dexsim_last_error()
    assert call(h, None, N, None, None, None, 0, 0, None, ps, pc, None) == 0                     # the body list is ignored without body_states
    torch.cuda.synchronize()
    assert (bits(os_.cpu().numpy()) == bits(c["site"])).all() and (bits(oc[:N].cpu().numpy()) == bits(c["cen"])).all()
    assert not ob.any()                                                        # none of the refused calls launched anything


@pytest.mark.gpu
def test_purity():
    import torch

    def calls(core):
        body, site, cen = gpu_fk(core, N)
        return [body, site, cen, gpu_fk(core, N, hand_frame=True, want=("site",))[1]]

    def between(core):
        gpu_fk(core, 3, env_ids=[69, 1, 64], bodies=[12, 18])
        gpu_fk(core, 100, q=torch.rand(100, NJ, device="cuda:0"), qd=torch.rand(100, NJ, device="cuda:0"), hand_frame=True)
        gpu_fk(core, 100, q=torch.rand(100, NJ, device="cuda:0"), bodies=[6], want=("body", "cen"))
    first = purity_frame(calls, between, n=N)
    assert not any(np.isnan(x).any() for x in first)


@pytest.mark.gpu
def test_public_surface():
    import torch
    from dexrobot_isaac_amd import make_env
    env = make_env("BlindGrasping", N, "cuda:0", "cuda:0", 0)
    env.reset()
    tip = "r_f_link1_tip"
    b = env.get_body_states(bodies=[tip, "right_hand_base"])                   # allocated by the call; names for bodies
    assert b.shape == (N, 2, 13) and not torch.isnan(b).any()
    idx = [env.model.body_names.index(tip), env.model.body_names.index("right_hand_base")]
    rbs = env.rigid_body_states[:, idx].cpu().numpy()                          # (refreshed on access)
    fr.check(fr.body_errors(b.cpu().numpy(), rbs, env.dof_vel.cpu().numpy()), "names against rigid_body_states")
    full, out = guarded(N, 2, 13)
    assert env.get_body_states(bodies=idx, out=out) is out and torch.equal(out, b)             # out= reuse
    guards_ok(full)
    full, out = guarded(N, NS, 7)
    allp = env.get_site_poses(out=out)
    guards_ok(full)
    assert allp.shape == (N, NS, 7) and allp.data_ptr() == out.data_ptr() and not torch.isnan(allp).any()
    for sites, sl in (("base", slice(0, 1)), ("tips", slice(1, 6)), ("pads", slice(6, 11))):
        part = env.get_site_poses(sites)
        assert part.shape == (N, sl.stop - sl.start, 7) and torch.equal(part, allp[:, sl])
    assert torch.equal(env.get_site_poses("tips", env_ids=[3, 1]), allp[[3, 1], 1:6])
    assert torch.equal(b[:, 0, 0:3], allp[:, 1, 0:3])                          # the tip body's origin is the tip site
    hand = env.get_site_poses("base", frame="hand")
    assert (hand - torch.tensor([0, 0, 0, 0, 0, 0, 1.0], device=hand.device)).abs().max() <= 1e-6
    full, out = guarded(N, 8)
    cen = env.get_centroid(out=out)
    guards_ok(full)
    assert cen["data"] is out and cen["com"].shape == (N, 3) and cen["kinetic"].shape == (N,) and not torch.isnan(out).any()
    assert torch.equal(env.get_centroid(q=env.dof_pos.clone(), qd=env.dof_vel.clone())["data"], out)   # the overrides at the current state
    assert not env.get_centroid(q=env.dof_pos.clone())["com_vel"].any()
    bad = env.get_site_poses("tips", env_ids=[5, -1, N, 69])                   # rows of ids out of range: NaN when the call allocated
    assert torch.isnan(bad[1:3]).all() and torch.equal(bad[[0, 3]], allp[[5, 69], 1:6])
    with pytest.raises(ValueError):
        env.get_body_states(bodies=["no_such_body"])
    with pytest.raises(ValueError):
        env.get_site_poses(sites="thumb")
    with pytest.raises(ValueError):
        env.get_centroid(qd=env.dof_vel.clone())
    env.close()
